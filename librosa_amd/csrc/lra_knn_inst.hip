// lra_knn_inst.hip -- the neighbour-graph kernels (lra_knn.h) and their launchers, a translation unit of its own so that it compiles side by
// side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#define LRA_KNN_KERNELS 1
#include "lra_knn.h"

#include "lra_knn_launch.h"

namespace lra {
namespace knn {

static unsigned blocks_of(long long count, int nt) { return (unsigned)((count + nt - 1) / nt); }

hipError_t launch_select(SelectArgs a, int rows, int tile, hipStream_t stream) {
    if (a.n <= 0 || a.m <= 0) return hipSuccess;
    a.g = geometry(rows, tile, a.k);
    if (a.g.lds == 0) return hipErrorInvalidValue;
    const long long grid = (a.n + a.g.rows - 1) / a.g.rows;
    if (grid > 0x7fffffffLL || a.n > 0x7fffffffLL || a.m > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    const SelectKernel kern = select_kernel(a.metric);
    if (!kern) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kNT), a.g.lds, stream, a);
    hipLaunchKernelGGL(knn_sort_rows, dim3((unsigned)a.n), dim3(kSortNT), 12 * a.k, stream, SortArgs{a.n, a.k, a.cnt, a.idx, a.dist});
    return hipGetLastError();
}

hipError_t launch_mutual(const MutualArgs& a, hipStream_t stream) {
    if (a.n * a.k > 0x7fffffffLL * kRowNT) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(knn_mutual, dim3(blocks_of(a.n * a.k, kRowNT)), dim3(kRowNT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_bandwidth(const BandwidthArgs& a, double* median, hipStream_t stream) {
    hipLaunchKernelGGL(knn_bandwidth, dim3((unsigned)a.n), dim3(kRowNT), 16 * (a.k + 1), stream, a);
    if (median) hipLaunchKernelGGL(knn_median, dim3(1), dim3(kMedNT), 0, stream, MedianArgs{a.dist_to_k, a.n, median, a.status});
    return hipGetLastError();
}

hipError_t launch_bw_check(const CheckArgs& a, hipStream_t stream) {
    if (a.count > 0x7fffffffLL * kRowNT) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(knn_bw_check, dim3(blocks_of(a.count, kRowNT)), dim3(kRowNT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_emit(const EmitArgs& a, hipStream_t stream) {
    const unsigned grid = blocks_of(a.n, kRowNT);
    if (!a.dense) {
        hipLaunchKernelGGL(knn_count, dim3(grid), dim3(kRowNT), 0, stream, a);
        hipLaunchKernelGGL(knn_scan, dim3(1), dim3(kRowNT), 0, stream, a);
    }
    hipLaunchKernelGGL(knn_emit, dim3(grid), dim3(kRowNT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_dense(const DenseArgs& a, hipStream_t stream) {
    const long long grid = ((a.n + kDenseTile - 1) / kDenseTile) * ((a.m + kDenseTile - 1) / kDenseTile);
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(knn_dense, dim3((unsigned)grid), dim3(kDenseNT), 0, stream, a);
    return hipGetLastError();
}

}  // namespace knn
}  // namespace lra
