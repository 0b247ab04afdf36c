// lra_yin_inst.hip -- instances and launcher of the YIN kernels (lra_yin.h) and the C entry points they serve, a translation unit of its own so that
// it compiles side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#include "lra_yin.h"

#include "lra_internal.h"
#include "lra_mixed_launch.h"

namespace lra {
namespace yin {

hipError_t launch_yin(const Args& a, long long batch, hipStream_t stream) {
    const long long grid = batch * a.groups;
    if (grid <= 0) return hipSuccess;
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    const int lds = lds_layout(a.N, a.max_period).total;
    if (lds > kYinLdsMax) return hipErrorInvalidConfiguration;
    void (*kern)(Args) = nullptr;
    switch (a.N) {
        case 0: kern = yin_kernel<0>; break;
#define LRA_YIN_CASE(N) \
    case N: kern = yin_kernel<N>; break;
        LRA_MIXED_SIZES(LRA_YIN_CASE)
#undef LRA_YIN_CASE
        default: return hipErrorInvalidValue;
    }
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kYinNT), lds, stream, a);
    return hipGetLastError();
}

}  // namespace yin
}  // namespace lra

// ---- C entry points: yin and the front half of pyin ----------------------------------------------------------------------------------------------
using namespace lra;

extern "C" {

static_assert(yin::kF0 == LRA_YIN_F0 && yin::kFrames == LRA_YIN_FRAMES, "yin codes");
static_assert(yin::transform_length(64, 27) == 160 && yin::transform_length(2048, 340) == 2400 && yin::transform_length(2048, 2047) == 4800 && yin::transform_length(4096, 705) == 0,
              "yin transform lengths");

int64_t lra_yin_lds_bytes(int frame_length, int max_period) {
    if (frame_length < 1 || max_period < 1) return 0;
    return yin::lds_layout(yin::transform_length(frame_length, max_period), max_period).total;
}

int lra_yin_exec(lra_ctx* ctx, const void* y, int64_t batch, int64_t n, int dtype, int frame_length, int hop_length, int center, int pad_mode, int min_period, int max_period,
                 double trough_threshold, double sr, int mode, void* f0, void* frames, void* shifts) {
    LRA_BIND(ctx);
    if (mode != LRA_YIN_F0 && mode != LRA_YIN_FRAMES) return fail(LRA_EINVAL, "yin: unknown mode");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "yin: dtype must be LRA_F32 or LRA_F64");
    if (frame_length < 3 || hop_length < 1) return fail(LRA_EINVAL, "yin: frame_length must be at least 3 and hop_length positive");
    if (pad_mode < 0 || pad_mode > 3) return fail(LRA_EINVAL, "yin: unknown pad mode");
    if (min_period < 1 || max_period <= min_period || max_period > frame_length - 1) return fail(LRA_EINVAL, "yin: need 1 <= min_period < max_period <= frame_length - 1");
    if (batch < 0 || n < 0) return fail(LRA_EINVAL, "yin: negative size");
    yin::Args a{};
    const int geometry = yin::prepare(a, n, frame_length, hop_length, center, pad_mode, min_period, max_period, trough_threshold, sr, mode);
    if (geometry == mixed::kGeometryTooShort)
        return fail(LRA_EINVAL, "yin: input is too short (n=" + std::to_string(n + 2 * (int64_t)a.pad) + ") for frame_length=" + std::to_string(frame_length));
    if (batch == 0) return LRA_OK;
    if (!y || (mode == LRA_YIN_F0 ? !f0 : (!frames || !shifts))) return fail(LRA_EINVAL, "null data pointer");
    if (a.n_frames > 0x7fffffffLL) return fail(LRA_EINVAL, "yin: too many frames per clip");
    if (geometry == mixed::kGeometryLds) return fail(LRA_EINVAL, "yin: max_period=" + std::to_string(max_period) + " does not fit the LDS of a workgroup");
    a.y = y;
    a.y_f64 = dtype == LRA_F64;
    if (a.N > 0) LRA_TRY(ctx_twiddles(ctx, a.N, LRA_F64, (const void**)&a.tw_m, (const void**)&a.tw_n));
    a.f0 = (double*)f0;
    a.frames = frames;
    a.shifts = shifts;
    if (batch * a.groups > 0x7fffffffLL) return fail(LRA_EINVAL, "yin: too many frames for one launch");
    LRA_HIP(yin::launch_yin(a, batch, ctx->stream));
    return LRA_OK;
}

}  // extern "C"
