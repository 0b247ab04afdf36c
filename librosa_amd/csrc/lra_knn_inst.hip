// lra_knn_inst.hip -- the neighbour-graph kernels (lra_knn.h) and their launchers and the C entry points they serve, a translation unit of its own so
// that it compiles side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#define LRA_KNN_KERNELS 1
#include "lra_knn.h"

#include "lra_internal.h"

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

// ---- C entry points: segment.cross_similarity and recurrence_matrix ------------------------------------------------------------------------------
using namespace lra;

extern "C" {

static_assert(knn::kMaxK == LRA_KNN_MAX_K && knn::kWorkBytes == LRA_KNN_WORK_BYTES, "knn limits");
static_assert(knn::kConnectivity == LRA_KNN_CONNECTIVITY && knn::kDistance == LRA_KNN_DISTANCE && knn::kAffinity == LRA_KNN_AFFINITY, "knn modes");
static_assert(knn::kBwScalar == LRA_KNN_BW_SCALAR && knn::kBwMeanK == LRA_KNN_BW_MEAN_K && knn::kBwGmeanK == LRA_KNN_BW_GMEAN_K && knn::kBwMeanKAvg == LRA_KNN_BW_MEAN_K_AVG &&
                  knn::kBwGmeanKAvg == LRA_KNN_BW_GMEAN_K_AVG && knn::kBwMeanKAvgPair == LRA_KNN_BW_MEAN_K_AVG_AND_PAIR && knn::kBwMatrix == LRA_KNN_BW_MATRIX,
              "knn bandwidth modes");
static_assert(knn::kStatusEmptyGraph == LRA_KNN_STATUS_EMPTY_GRAPH && knn::kStatusRowEmpty == LRA_KNN_STATUS_ROW_EMPTY && knn::kStatusNonPositive == LRA_KNN_STATUS_NON_POSITIVE,
              "knn status bits");
static_assert(knn::geometry(0, 0, 1024).lds > 0 && knn::geometry(0, 0, knn::kMaxK).lds > 0 && knn::geometry(0, 0, knn::kMaxK).lds <= knn::kLdsMax, "knn: the longest list is served");

int64_t lra_knn_lds_bytes(int rows, int tile, int k) { return knn::geometry(rows, tile, k).lds; }

// the work area: the status word, the lowest empty row, the scalar bandwidth, the entry count
struct KnnWork {
    int status, first_empty;
    double bandwidth;
    long long total;
};
static_assert(sizeof(KnnWork) <= LRA_KNN_WORK_BYTES, "knn work area");

static bool knn_fill_value(knn::Value* v, int mode, int bw_mode, double bw_scalar, int bw_on_device, const void* sigma, const void* matrix, int64_t m, void* work, std::string* why) {
    if (mode < LRA_KNN_CONNECTIVITY || mode > LRA_KNN_AFFINITY) return *why = "knn: unknown mode", false;
    if (bw_mode < LRA_KNN_BW_SCALAR || bw_mode > LRA_KNN_BW_MATRIX) return *why = "knn: unknown bandwidth mode", false;
    v->mode = mode;
    v->bw_mode = bw_mode;
    v->bw_scalar = bw_scalar;
    v->bw_ptr = bw_on_device ? &((const KnnWork*)work)->bandwidth : nullptr;
    v->sigma = (const double*)sigma;
    v->matrix = (const double*)matrix;
    v->m = m;
    if (mode == LRA_KNN_AFFINITY) {
        if (bw_mode == LRA_KNN_BW_MATRIX ? !matrix : (bw_mode != LRA_KNN_BW_SCALAR && !sigma)) return *why = "knn: the bandwidth mode's table is missing", false;
        if (bw_on_device && !work) return *why = "null data pointer", false;
    }
    return true;
}

int lra_knn_select_exec(lra_ctx* ctx, const void* Q, const void* R, int dtype, int64_t n_features, int64_t n, int64_t m, int metric, int k, int64_t width, int skip_zero, int rows, int tile,
                        void* count, void* index, void* distance) {
    LRA_BIND(ctx);
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "knn: the features must be LRA_F32 or LRA_F64");
    if (metric < LRA_DTW_EUCLIDEAN || metric > LRA_DTW_COSINE) return fail(LRA_EINVAL, "knn: unknown metric");
    if (n_features < 1 || n < 1 || m < 1) return fail(LRA_EINVAL, "knn: need at least one feature and one frame of each sequence");
    if (n > 0x7fffffffLL || m > 0x7fffffffLL) return fail(LRA_EINVAL, "knn: too many frames");
    if (k < 1 || k > LRA_KNN_MAX_K) return fail(LRA_EINVAL, "knn: k must be between 1 and LRA_KNN_MAX_K = " + std::to_string(LRA_KNN_MAX_K));
    if (width < 0) return fail(LRA_EINVAL, "knn: negative width");
    if (lra_knn_lds_bytes(rows, tile, k) == 0)
        return fail(LRA_EINVAL, "knn: rows is 0 (the library's choice) or a power of two up to 16, tile 0 or a power of two from 4 to 1024, rows * tile at most 2048, and the lists must fit the LDS");
    if (!Q || !R || !count || !index || !distance) return fail(LRA_EINVAL, "null data pointer");
    knn::SelectArgs a{};
    a.Q = Q;
    a.R = R;
    a.f64 = dtype == LRA_F64;
    a.metric = metric;
    a.d = n_features;
    a.n = n;
    a.m = m;
    a.k = k;
    a.width = width;
    a.skip_zero = skip_zero != 0;
    a.cnt = (int*)count;
    a.idx = (int*)index;
    a.dist = (double*)distance;
    LRA_HIP(knn::launch_select(a, rows, tile, ctx->stream));
    return LRA_OK;
}

int lra_knn_mutual_exec(lra_ctx* ctx, int64_t n, int k, const void* count, const void* index, const void* distance, int sym, int drop_zero, void* keep) {
    LRA_BIND(ctx);
    if (n < 1 || k < 1) return fail(LRA_EINVAL, "knn: the lists are empty");
    if (!count || !index || !distance || !keep) return fail(LRA_EINVAL, "null data pointer");
    LRA_HIP(knn::launch_mutual(knn::MutualArgs{n, k, (const int*)count, (const int*)index, (const double*)distance, sym != 0, drop_zero != 0, (uint8_t*)keep}, ctx->stream));
    return LRA_OK;
}

// the status word and the lowest empty row, read back (this waits for the stream)
static int knn_read_status(lra_ctx* ctx, const void* work, int* status, int64_t* first_empty) {
    KnnWork h{};
    LRA_TRY(read_status(ctx, work, &h, sizeof(h)));
    *status = h.status;
    if (first_empty) *first_empty = h.first_empty;
    return LRA_OK;
}

int lra_knn_bandwidth_exec(lra_ctx* ctx, int64_t n, int k, const void* count, const void* distance, const void* keep, int add_self, int bandwidth_k, int median, void* dist_to_k, void* avg,
                           void* work, int* status, int64_t* first_empty) {
    LRA_BIND(ctx);
    if (n < 1 || k < 1 || bandwidth_k < 1) return fail(LRA_EINVAL, "knn: the lists are empty, or bandwidth_k is not positive");
    if (n > 0x7fffffffLL) return fail(LRA_EINVAL, "knn: too many frames");
    if (!count || !distance || !dist_to_k || !avg || !work || !status || !first_empty) return fail(LRA_EINVAL, "null data pointer");
    const KnnWork init{0, 0x7fffffff, 0.0, 0};
    LRA_HIP(hipMemcpyAsync(work, &init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
    LRA_HIP(hipStreamSynchronize(ctx->stream));   // (init lives on this frame)
    KnnWork* w = (KnnWork*)work;
    knn::BandwidthArgs a{n, k, (const int*)count, (const double*)distance, (const uint8_t*)keep, add_self != 0, bandwidth_k, (double*)dist_to_k, (double*)avg, &w->status};
    LRA_HIP(knn::launch_bandwidth(a, median ? &w->bandwidth : nullptr, ctx->stream));
    return knn_read_status(ctx, work, status, first_empty);
}

int lra_knn_bw_check_exec(lra_ctx* ctx, const void* matrix, int64_t count, void* work, int* status) {
    LRA_BIND(ctx);
    if (count < 1) return fail(LRA_EINVAL, "knn: the bandwidth matrix is empty");
    if (!matrix || !work || !status) return fail(LRA_EINVAL, "null data pointer");
    LRA_HIP(hipMemsetAsync(work, 0, sizeof(KnnWork), ctx->stream));
    LRA_HIP(knn::launch_bw_check(knn::CheckArgs{(const double*)matrix, count, &((KnnWork*)work)->status}, ctx->stream));
    return knn_read_status(ctx, work, status, nullptr);
}

int lra_knn_emit_exec(lra_ctx* ctx, int64_t n, int64_t m, int k, const void* count, const void* index, const void* distance, const void* keep, int self, int mode, int bw_mode,
                      double bw_scalar, int bw_on_device, const void* sigma, const void* matrix, void* work, void* counts, void* indptr, void* indices, void* data, void* dense,
                      int64_t* total) {
    LRA_BIND(ctx);
    if (n < 1 || m < 1 || k < 1) return fail(LRA_EINVAL, "knn: the lists are empty");
    if (n * ((int64_t)k + 1) > 0x7fffffffLL) return fail(LRA_EINVAL, "knn: more entries than an int32 index array addresses");
    if (!count || !index || !distance || !keep || !work) return fail(LRA_EINVAL, "null data pointer");
    if (dense ? false : (!counts || !indptr || !indices || !data || !total)) return fail(LRA_EINVAL, "null data pointer");
    knn::EmitArgs a{};
    std::string why;
    if (!knn_fill_value(&a.val, mode, bw_mode, bw_scalar, bw_on_device, sigma, matrix, m, work, &why)) return fail(LRA_EINVAL, why);
    a.n = n;
    a.m = m;
    a.k = k;
    a.cnt = (const int*)count;
    a.idx = (const int*)index;
    a.dist = (const double*)distance;
    a.keep = (const uint8_t*)keep;
    a.self = self != 0;
    a.counts = (int*)counts;
    a.indptr = dense ? nullptr : (int*)indptr;
    a.indices = (int*)indices;
    a.data = data;
    a.dense = dense;
    a.total = &((KnnWork*)work)->total;
    if (dense) LRA_HIP(hipMemsetAsync(dense, 0, (size_t)n * (size_t)m * (mode == LRA_KNN_CONNECTIVITY ? 1 : 8), ctx->stream));
    LRA_HIP(knn::launch_emit(a, ctx->stream));
    if (!dense) {
        long long h = 0;
        LRA_TRY(read_status(ctx, a.total, &h, sizeof(h)));
        *total = h;
    }
    return LRA_OK;
}

int lra_knn_dense_exec(lra_ctx* ctx, const void* Q, const void* R, int dtype, int64_t n_features, int64_t n, int64_t m, int metric, int64_t width, int self, int mode, int bw_mode,
                       double bw_scalar, int bw_on_device, const void* sigma, const void* matrix, void* work, void* out) {
    LRA_BIND(ctx);
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "knn: the features must be LRA_F32 or LRA_F64");
    if (metric < LRA_DTW_EUCLIDEAN || metric > LRA_DTW_COSINE) return fail(LRA_EINVAL, "knn: unknown metric");
    if (n_features < 1 || n < 1 || m < 1) return fail(LRA_EINVAL, "knn: need at least one feature and one frame of each sequence");
    if (width < 0) return fail(LRA_EINVAL, "knn: negative width");
    if (!Q || !R || !out) return fail(LRA_EINVAL, "null data pointer");
    knn::DenseArgs a{};
    std::string why;
    if (!knn_fill_value(&a.val, mode, bw_mode, bw_scalar, bw_on_device, sigma, matrix, m, work, &why)) return fail(LRA_EINVAL, why);
    a.Q = Q;
    a.R = R;
    a.f64 = dtype == LRA_F64;
    a.metric = metric;
    a.d = n_features;
    a.n = n;
    a.m = m;
    a.width = width;
    a.self = self != 0;
    a.out = out;
    LRA_HIP(knn::launch_dense(a, ctx->stream));
    return LRA_OK;
}

}  // extern "C"
