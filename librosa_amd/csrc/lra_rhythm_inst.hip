// lra_rhythm_inst.hip -- instances and launchers of the tempogram kernels (lra_rhythm.h) and the C entry points they serve, a translation unit of its
// own so that it compiles side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#include "lra_rhythm.h"

#include "lra_internal.h"
#include "lra_mixed_launch.h"

namespace lra {
namespace rhythm {

hipError_t launch_tempogram(const Args& a, long long batch, hipStream_t stream) {
    const long long grid = batch * a.groups;
    if (grid <= 0) return hipSuccess;
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    const int lds = lds_layout(a.N, a.W, a.mode, a.tile != 0).total;
    if (lds > kRhythmLdsMax) return hipErrorInvalidConfiguration;
    void (*kern)(Args) = nullptr;
    switch (a.N) {
        case 0: kern = tempogram_kernel<0>; break;
#define LRA_RHYTHM_CASE(N) \
    case N: kern = tempogram_kernel<N>; break;
        LRA_MIXED_SIZES(LRA_RHYTHM_CASE)
#undef LRA_RHYTHM_CASE
        default: return hipErrorInvalidValue;
    }
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kRhythmNT), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_tempo_finish(const FinishArgs& a, long long batch, hipStream_t stream) {
    if (batch <= 0) return hipSuccess;
    if (batch > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(tempo_mean_finish_kernel<double>, dim3((unsigned)batch), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rhythm
}  // namespace lra

// ---- C entry points: tempogram / tempo -----------------------------------------------------------------------------------------------------------
using namespace lra;

extern "C" {

static_assert(rhythm::kWrite == LRA_TEMPOGRAM_WRITE && rhythm::kSum == LRA_TEMPOGRAM_SUM && rhythm::kArgmax == LRA_TEMPOGRAM_ARGMAX && rhythm::kNormNone == LRA_TEMPOGRAM_NORM_NONE &&
                  rhythm::kNormInf == LRA_TEMPOGRAM_NORM_INF && rhythm::kNormL1 == LRA_TEMPOGRAM_NORM_L1 && rhythm::kNormL2 == LRA_TEMPOGRAM_NORM_L2,
              "tempogram codes");
static_assert(rhythm::transform_length(344) == 720 && rhythm::transform_length(384) == 800 && rhythm::transform_length(689) == 1440 && rhythm::transform_length(800) == 1600 &&
                  rhythm::transform_length(2400) == 4800 && rhythm::transform_length(2401) == 0,
              "tempogram transform lengths");

int64_t lra_tempogram_work_bytes(int64_t batch, int64_t n_frames, int win_length, int mode) {
    const int64_t groups = n_frames > 0 ? (n_frames + rhythm::kRhythmGroup - 1) / rhythm::kRhythmGroup : 0;
    return 16 + (mode == LRA_TEMPOGRAM_SUM && batch > 0 && win_length > 0 ? batch * groups * (int64_t)win_length * 8 : 0);
}

int lra_tempogram_exec(lra_ctx* ctx, const void* env, int64_t batch, int64_t n, int dtype, int win_length, int center, const void* window, int norm, int mode,
                       const void* logprior, const void* bpms, void* out, void* work, int* nonfinite) {
    LRA_BIND(ctx);
    if (nonfinite) *nonfinite = 0;
    if (mode < LRA_TEMPOGRAM_WRITE || mode > LRA_TEMPOGRAM_ARGMAX) return fail(LRA_EINVAL, "tempogram: unknown mode");
    if (norm < LRA_TEMPOGRAM_NORM_NONE || norm > LRA_TEMPOGRAM_NORM_L2) return fail(LRA_EINVAL, "tempogram: unknown norm code");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "tempogram: dtype must be LRA_F32 or LRA_F64");
    if (win_length < 1) return fail(LRA_EINVAL, "tempogram: win_length must be a positive integer");
    if (batch < 0 || n < 0) return fail(LRA_EINVAL, "tempogram: negative size");
    rhythm::Args a{};
    const int geometry = rhythm::prepare(a, n, win_length, center, norm, mode);
    if (geometry == mixed::kGeometryTooShort)
        return fail(LRA_EINVAL, "tempogram: input is too short (n=" + std::to_string(n + 2 * (int64_t)a.pad) + ") for frame_length=" + std::to_string(win_length));
    const int64_t n_frames = a.n_frames;
    if (batch == 0 || n_frames == 0) return LRA_OK;
    if (!env || !window || !out || !work) return fail(LRA_EINVAL, "null data pointer");
    if (mode != LRA_TEMPOGRAM_WRITE && (!logprior || !bpms)) return fail(LRA_EINVAL, "tempogram: tempo modes need the prior and the BPM table");
    if (n_frames > 0x7fffffffLL) return fail(LRA_EINVAL, "tempogram: too many frames per clip");
    if (geometry == mixed::kGeometryLds) return fail(LRA_EINVAL, "tempogram: win_length=" + std::to_string(win_length) + " does not fit the LDS of a workgroup");
    a.env = env;
    a.env_f64 = dtype == LRA_F64;
    a.win = (const double*)window;
    if (a.N > 0) LRA_TRY(ctx_twiddles(ctx, a.N, LRA_F64, (const void**)&a.tw_m, (const void**)&a.tw_n));
    a.logprior = (const double*)logprior;
    a.bpms = (const double*)bpms;
    a.out = (double*)out;
    a.flag = (int*)work;
    a.partial = (double*)((char*)work + 16);
    if (batch * a.groups > 0x7fffffffLL) return fail(LRA_EINVAL, "tempogram: too many frames for one launch");
    LRA_HIP(hipMemsetAsync(work, 0, sizeof(int), ctx->stream));
    LRA_HIP(rhythm::launch_tempogram(a, batch, ctx->stream));
    if (mode == LRA_TEMPOGRAM_SUM) {
        rhythm::FinishArgs f{a.partial, a.logprior, a.bpms, a.out, n_frames, a.groups, win_length};
        LRA_HIP(rhythm::launch_tempo_finish(f, batch, ctx->stream));
    }
    if (nonfinite) {
        int h = 0;
        LRA_TRY(read_status(ctx, work, &h, sizeof(int)));
        *nonfinite = h != 0;
    }
    return LRA_OK;
}

}  // extern "C"
