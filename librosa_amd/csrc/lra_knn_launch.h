// lra_knn_launch.h -- what lra_api.hip sees of the neighbour-graph kernels (lra_knn.h): the launchers (defined in lra_knn_inst.hip, a
// translation unit of its own).
#pragma once

#include <hip/hip_runtime.h>

#include "lra_knn.h"

namespace lra {
namespace knn {
// the selection and the sort of every row by index (a.g is set here); rows, tile: 0 for the library's choice
hipError_t launch_select(SelectArgs a, int rows, int tile, hipStream_t stream);
hipError_t launch_mutual(const MutualArgs& a, hipStream_t stream);
// the per-row statistics and, with `median`, np.nanmedian(dist_to_k) into *median
hipError_t launch_bandwidth(const BandwidthArgs& a, double* median, hipStream_t stream);
hipError_t launch_bw_check(const CheckArgs& a, hipStream_t stream);
// count, scan (for the sparse arrays) and emit
hipError_t launch_emit(const EmitArgs& a, hipStream_t stream);
hipError_t launch_dense(const DenseArgs& a, hipStream_t stream);
}  // namespace knn
}  // namespace lra
