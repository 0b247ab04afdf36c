// lra_dtw_inst.hip -- the DTW kernels (lra_dtw.h) and their launchers and the C entry points they serve, a translation unit of its own so that it
// compiles side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#define LRA_DTW_KERNELS 1
#include "lra_dtw.h"

#include "lra_internal.h"

namespace lra {
namespace dtw {

static bool grid_fits(long long grid) { return grid > 0 && grid <= 0x7fffffffLL; }

hipError_t launch_cost(const CostArgs& a, hipStream_t stream) {
    if (a.N <= 0 || a.M <= 0) return hipSuccess;
    const long long grid = ((a.N + kCostTile - 1) / kCostTile) * ((a.M + kCostTile - 1) / kCostTile);
    if (!grid_fits(grid)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(dtw_cost, dim3((unsigned)grid), dim3(kCostNT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_prepare(const PrepArgs& a, hipStream_t stream) {
    if (a.count <= 0) return hipSuccess;
    const long long grid = (a.count + kPrepNT - 1) / kPrepNT;
    if (!grid_fits(grid)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(dtw_prepare, dim3((unsigned)grid), dim3(kPrepNT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_widen(const WidenArgs& a, hipStream_t stream) {
    if (a.count <= 0) return hipSuccess;
    const long long grid = (a.count + kPrepNT - 1) / kPrepNT;
    if (!grid_fits(grid)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(dtw_widen, dim3((unsigned)grid), dim3(kPrepNT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_accumulate(AccArgs a, int tile, hipStream_t stream) {
    if (a.N <= 0 || a.M <= 0) return hipSuccess;
    if (tile != 0 && !tile_ok(tile)) return hipErrorInvalidValue;
    if (a.st.n < 1 || a.st.n > kMaxSteps || a.st.max0 < 0 || a.st.max0 > kMaxStep || a.st.max1 < 0 || a.st.max1 > kMaxStep) return hipErrorInvalidValue;
    a.g = geometry(tile, a.st.max0, a.st.max1);
    if (a.g.lds > kLdsMax) return hipErrorInvalidConfiguration;
    a.tiles_n = (a.N + a.g.tile - 1) / a.g.tile;
    a.tiles_m = (a.M + a.g.tile - 1) / a.g.tile;
    void (*kern)(AccArgs) = a.st.n == 3 ? dtw_accumulate : dtw_accumulate_any;
    if (a.g.lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, a.g.lds);
        if (e != hipSuccess) return e;
    }
    for (long long diag = 0; diag < a.tiles_n + a.tiles_m - 1; ++diag) {
        const long long grid = diag_tiles(diag, a.tiles_n, a.tiles_m).count;
        if (!grid_fits(grid)) return hipErrorInvalidConfiguration;
        a.diag = diag;
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kAccNT), a.g.lds, stream, a);
    }
    return hipGetLastError();
}

hipError_t launch_backtrack(const BackArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(dtw_backtrack, dim3(1), dim3(kBackNT), 0, stream, a);
    return hipGetLastError();
}

}  // namespace dtw
}  // namespace lra

// ---- C entry points: sequence.dtw and dtw_backtracking -------------------------------------------------------------------------------------------
using namespace lra;

extern "C" {

static_assert(dtw::kEuclidean == LRA_DTW_EUCLIDEAN && dtw::kSqeuclidean == LRA_DTW_SQEUCLIDEAN && dtw::kCityblock == LRA_DTW_CITYBLOCK && dtw::kCosine == LRA_DTW_COSINE, "dtw metrics");
static_assert(dtw::kF32 == LRA_F32 && dtw::kF64 == LRA_F64 && dtw::kI32 == LRA_DTW_I32 && dtw::kI64 == LRA_DTW_I64 && dtw::kU8 == LRA_DTW_U8, "dtw types");
static_assert(dtw::kFlagNan == LRA_DTW_FLAG_NAN && dtw::kFlagEndInf == LRA_DTW_FLAG_END_INF && dtw::kFlagRowInf == LRA_DTW_FLAG_ROW_INF &&
                  dtw::kFlagNotOrigin == LRA_DTW_FLAG_NOT_ORIGIN && dtw::kFlagBadStep == LRA_DTW_FLAG_BAD_STEP,
              "dtw flags");
static_assert(dtw::kMaxSteps == LRA_DTW_MAX_STEPS && dtw::kMaxStep == LRA_DTW_MAX_STEP && dtw::kStartEnd == LRA_DTW_START_END && dtw::kStartArgmin == LRA_DTW_START_ARGMIN, "dtw limits");
static_assert(dtw::geometry(64, dtw::kMaxStep, dtw::kMaxStep).lds <= dtw::kLdsMax, "dtw: the largest tile with the widest halo fits");

int64_t lra_dtw_lds_bytes(int tile, int max_0, int max_1) {
    if ((tile != 0 && !dtw::tile_ok(tile)) || max_0 < 0 || max_1 < 0 || max_0 > dtw::kMaxStep || max_1 > dtw::kMaxStep) return 0;
    return dtw::geometry(tile, max_0, max_1).lds;
}

// the step table of a call (host arrays) as the kernels take it; false where it breaks a limit
static bool dtw_step_table(const int32_t* steps, const double* w_add, const double* w_mul, int n_steps, dtw::StepTable* st, std::string* why) {
    if (!steps || n_steps < 1 || n_steps > dtw::kMaxSteps) {
        *why = "dtw: the step table holds 1 to " + std::to_string(dtw::kMaxSteps) + " steps";
        return false;
    }
    *st = dtw::StepTable{};
    st->n = n_steps;
    for (int i = 0; i < n_steps; ++i) {
        const int s0 = steps[2 * i], s1 = steps[2 * i + 1];
        if (s0 < 0 || s1 < 0 || s0 > dtw::kMaxStep || s1 > dtw::kMaxStep || (s0 == 0 && s1 == 0)) {
            *why = "dtw: a step component lies in 0 .. " + std::to_string(dtw::kMaxStep) + " and no step is (0, 0)";
            return false;
        }
        st->s0[i] = s0;
        st->s1[i] = s1;
        st->w_add[i] = w_add ? w_add[i] : 0.0;
        st->w_mul[i] = w_mul ? w_mul[i] : 1.0;
        if (s0 > st->max0) st->max0 = s0;
        if (s1 > st->max1) st->max1 = s1;
    }
    return true;
}

// the flag word of a stage, read back (this waits for the stream)

int lra_dtw_cost_exec(lra_ctx* ctx, const void* X, const void* Y, int dtype, int64_t n_features, int64_t N, int64_t M, int metric, void* C, void* work, int* flags) {
    LRA_BIND(ctx);
    if (flags) *flags = 0;
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "dtw: the features must be LRA_F32 or LRA_F64");
    if (metric < LRA_DTW_EUCLIDEAN || metric > LRA_DTW_COSINE) return fail(LRA_EINVAL, "dtw: unknown metric");
    if (n_features < 1 || N < 1 || M < 1) return fail(LRA_EINVAL, "dtw: need at least one feature and one frame of each sequence");
    if (!X || !Y || !C || !work) return fail(LRA_EINVAL, "null data pointer");
    dtw::CostArgs a{X, Y, dtype == LRA_F64, metric, n_features, N, M, (double*)C, (int*)work};
    LRA_HIP(hipMemsetAsync(work, 0, sizeof(int), ctx->stream));
    LRA_HIP(dtw::launch_cost(a, ctx->stream));
    return flags ? read_status(ctx, work, flags, sizeof(int)) : LRA_OK;
}

int lra_dtw_prepare_exec(lra_ctx* ctx, const void* C, int dtype, int64_t count, void* out, void* work, int* flags) {
    LRA_BIND(ctx);
    if (flags) *flags = 0;
    if (dtype != LRA_F32 && dtype != LRA_F64 && dtype != LRA_DTW_I32 && dtype != LRA_DTW_I64 && dtype != LRA_DTW_U8) return fail(LRA_EINVAL, "dtw: unknown type of C");
    if (count < 1) return fail(LRA_EINVAL, "dtw: C is empty");
    if (!C || !work || (!out && dtype != LRA_F64)) return fail(LRA_EINVAL, "null data pointer");
    dtw::PrepArgs a{C, dtype, count, (double*)out, (int*)work};
    LRA_HIP(hipMemsetAsync(work, 0, sizeof(int), ctx->stream));
    LRA_HIP(dtw::launch_prepare(a, ctx->stream));
    return flags ? read_status(ctx, work, flags, sizeof(int)) : LRA_OK;
}

int lra_dtw_accumulate_exec(lra_ctx* ctx, const void* C, int64_t N, int64_t M, const int32_t* steps, const double* weights_add, const double* weights_mul, int n_steps, int subseq, int band,
                            int64_t band_lo, int64_t band_hi, int tile, void* D, void* step_idx) {
    LRA_BIND(ctx);
    if (N < 1 || M < 1) return fail(LRA_EINVAL, "dtw: C is empty");
    if (tile != 0 && !dtw::tile_ok(tile)) return fail(LRA_EINVAL, "dtw: tile is 0 (the library's choice), 8, 16, 32 or 64");
    if (!C || !D || !step_idx) return fail(LRA_EINVAL, "null data pointer");
    dtw::AccArgs a{};
    std::string why;
    if (!dtw_step_table(steps, weights_add, weights_mul, n_steps, &a.st, &why)) return fail(LRA_EINVAL, why);
    a.C = (const double*)C;
    a.N = N;
    a.M = M;
    a.subseq = subseq != 0;
    a.band = band != 0;
    a.band_lo = band_lo;
    a.band_hi = band_hi;
    a.D = (double*)D;
    a.steps = (uint8_t*)step_idx;
    LRA_HIP(dtw::launch_accumulate(a, tile, ctx->stream));
    return LRA_OK;
}

int lra_dtw_widen_exec(lra_ctx* ctx, const void* step_idx, int64_t count, void* out) {
    LRA_BIND(ctx);
    if (count < 0) return fail(LRA_EINVAL, "dtw: negative size");
    if (count == 0) return LRA_OK;
    if (!step_idx || !out) return fail(LRA_EINVAL, "null data pointer");
    LRA_HIP(dtw::launch_widen(dtw::WidenArgs{(const uint8_t*)step_idx, count, (int*)out}, ctx->stream));
    return LRA_OK;
}

int lra_dtw_backtrack_exec(lra_ctx* ctx, const void* D, const void* step_idx, int steps_i32, int64_t N, int64_t M, const int32_t* steps, int n_steps, int subseq, int64_t start, void* path,
                           void* work, int64_t* length, int* status) {
    LRA_BIND(ctx);
    if (N < 1 || M < 1) return fail(LRA_EINVAL, "dtw: the step matrix is empty");
    if (!step_idx || !path || !work || !length || !status) return fail(LRA_EINVAL, "null data pointer");
    if (start < LRA_DTW_START_ARGMIN || start >= M) return fail(LRA_EINVAL, "dtw: start is a column of the matrix, LRA_DTW_START_END or LRA_DTW_START_ARGMIN");
    if (start == LRA_DTW_START_ARGMIN && !D) return fail(LRA_EINVAL, "dtw: LRA_DTW_START_ARGMIN needs D");
    dtw::BackArgs a{};
    std::string why;
    if (!dtw_step_table(steps, nullptr, nullptr, n_steps, &a.st, &why)) return fail(LRA_EINVAL, why);
    a.D = (const double*)D;
    a.steps = step_idx;
    a.steps_i32 = steps_i32 != 0;
    a.N = N;
    a.M = M;
    a.subseq = subseq != 0;
    a.start = start;
    a.path = (long long*)path;
    a.cap = N + M - 1;
    a.length = (long long*)work;
    a.status = (int*)((char*)work + 8);
    LRA_HIP(dtw::launch_backtrack(a, ctx->stream));
    struct { long long length; int status; int pad; } h{};
    LRA_TRY(read_status(ctx, work, &h, 16));
    *length = h.length;
    *status = h.status;
    return LRA_OK;
}

}  // extern "C"
