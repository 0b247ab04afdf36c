// lra_peaks_inst.hip -- instances and the launchers of the peak-picking kernels (lra_peaks.h) and the C entry points they serve, a translation unit
// of its own so that it compiles side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#include "lra_peaks.h"

#include "lra_internal.h"

namespace lra {
namespace peaks {

template <class T> static hipError_t launch_typed(const Args& a, long long batch, hipStream_t stream) {
    const long long tiles = (a.n + kTile - 1) / kTile;
    if (batch > 0x7fffffffLL || tiles * batch > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(peak_stats_kernel<T>, dim3((unsigned)batch), dim3(kStatsNT), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(peak_candidates_kernel<T>, dim3((unsigned)(tiles * batch)), dim3(kTile), 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.method == kGreedy) hipLaunchKernelGGL(peak_greedy_kernel<T>, dim3((unsigned)batch), dim3(kWave), 0, stream, a);
    else hipLaunchKernelGGL(peak_dp_kernel<T>, dim3((unsigned)batch), dim3(kWave), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_peak_pick(const Args& a, long long batch, bool f64, hipStream_t stream) {
    if (batch <= 0 || a.n <= 0) return hipSuccess;
    return f64 ? launch_typed<double>(a, batch, stream) : launch_typed<float>(a, batch, stream);
}

hipError_t launch_prev_minimum(const MinArgs& a, long long batch, bool f64, hipStream_t stream) {
    if (batch <= 0 || a.m <= 0) return hipSuccess;
    if (batch > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    if (f64) hipLaunchKernelGGL(prev_minimum_kernel<double>, dim3((unsigned)batch), dim3(kWave), 0, stream, a);
    else hipLaunchKernelGGL(prev_minimum_kernel<float>, dim3((unsigned)batch), dim3(kWave), 0, stream, a);
    return hipGetLastError();
}

}  // namespace peaks
}  // namespace lra

// ---- C entry points: peak picking and onset backtracking -----------------------------------------------------------------------------------------
using namespace lra;

extern "C" {

static_assert(peaks::kGreedy == LRA_PEAK_GREEDY && peaks::kDpCount == LRA_PEAK_DP_COUNT && peaks::kDpValue == LRA_PEAK_DP_VALUE, "peak codes");

namespace {
struct PeakWork {
    int64_t status, norm, cand, values, taken, total;
};
PeakWork peak_work_layout(int64_t batch, int64_t n, int method) {
    auto up = [](int64_t b) { return (b + 255) / 256 * 256; };
    const int64_t rows = batch > 0 ? batch : 0, len = n > 0 ? n : 0, cells = rows * len;
    const bool dp = method != LRA_PEAK_GREEDY;
    PeakWork w{};
    w.status = 0;
    w.norm = 256;
    w.cand = w.norm + up(cells * 8);
    w.values = w.cand + up(cells);
    w.taken = w.values + up(dp ? rows * (len + 1) * 8 : 0);
    w.total = w.taken + up(dp ? rows * ((len + 63) / 64) * 8 : 0);
    return w;
}
}  // namespace

int64_t lra_peak_pick_work_bytes(int64_t batch, int64_t n, int method) { return peak_work_layout(batch, n, method).total; }

int lra_peak_pick_exec(lra_ctx* ctx, const void* x, int64_t batch, int64_t n, int dtype, int normalize, int64_t pre_max, int64_t post_max, int64_t pre_avg, int64_t post_avg,
                       double delta, int64_t wait, int method, void* out, void* norm_out, void* work, int* status) {
    LRA_BIND(ctx);
    if (status) *status = 0;
    if (method != LRA_PEAK_GREEDY && method != LRA_PEAK_DP_COUNT && method != LRA_PEAK_DP_VALUE) return fail(LRA_EINVAL, "peak_pick: unknown method");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "peak_pick: dtype must be LRA_F32 or LRA_F64");
    if (batch < 0 || n < 0) return fail(LRA_EINVAL, "peak_pick: negative size");
    if (pre_max < 0 || pre_avg < 0 || wait < 0 || !(delta >= 0)) return fail(LRA_EINVAL, "peak_pick: pre_max, pre_avg, delta and wait must be non-negative");
    if (post_max <= 0 || post_avg <= 0) return fail(LRA_EINVAL, "peak_pick: post_max and post_avg must be positive");
    if (batch == 0 || n == 0) {
        if (status) *status = LRA_PEAK_ALL_FINITE;
        return LRA_OK;
    }
    if (!x || !out || !work) return fail(LRA_EINVAL, "null data pointer");
    if (n > 0x7fffffffLL - 64) return fail(LRA_EINVAL, "peak_pick: too many frames per row");
    const PeakWork w = peak_work_layout(batch, n, method);
    char* base = (char*)work;
    peaks::Args a{};
    a.x = x;
    a.n = n;
    a.normalize = normalize != 0;
    a.pre_max = (int)peaks::clamp_window(pre_max, n);
    a.post_max = (int)peaks::clamp_window(post_max, n);
    a.pre_avg = (int)peaks::clamp_window(pre_avg, n);
    a.post_avg = (int)peaks::clamp_window(post_avg, n);
    a.wait = (int)peaks::clamp_window(wait, n);
    a.delta = delta;
    a.method = method;
    a.status = (int*)(base + w.status);
    a.norm = norm_out ? norm_out : base + w.norm;
    a.cand = (unsigned char*)(base + w.cand);
    a.values = (double*)(base + w.values);
    a.taken = (unsigned long long*)(base + w.taken);
    a.out = (unsigned char*)out;
    LRA_HIP(hipMemsetAsync(work, 0, 2 * sizeof(int), ctx->stream));
    LRA_HIP(peaks::launch_peak_pick(a, batch, dtype == LRA_F64, ctx->stream));
    if (status) {
        int h[2] = {0, 0};
        LRA_TRY(read_status(ctx, work, h, sizeof(h)));
        *status = (h[0] ? LRA_PEAK_ANY_NONZERO : 0) | (h[1] ? 0 : LRA_PEAK_ALL_FINITE);
    }
    return LRA_OK;
}

int lra_prev_minimum_exec(lra_ctx* ctx, const void* energy, int64_t batch, int64_t m, int dtype, void* out) {
    LRA_BIND(ctx);
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "prev_minimum: dtype must be LRA_F32 or LRA_F64");
    if (batch < 0 || m < 0) return fail(LRA_EINVAL, "prev_minimum: negative size");
    if (batch == 0 || m == 0) return LRA_OK;
    if (!energy || !out) return fail(LRA_EINVAL, "null data pointer");
    if (m > 0x7fffffffLL - 64) return fail(LRA_EINVAL, "prev_minimum: too many frames per row");
    peaks::MinArgs a{energy, m, (int*)out};
    LRA_HIP(peaks::launch_prev_minimum(a, batch, dtype == LRA_F64, ctx->stream));
    return LRA_OK;
}

}  // extern "C"
