// lra_chroma_inst.hip -- instances and the launcher of the chroma kernels (lra_chroma.h) and the C entry points they serve, a translation unit of its
// own so that it compiles side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#include "lra_chroma.h"

#include "lra_internal.h"

namespace lra {
namespace chroma {

template <class T> static hipError_t launch_typed(Args a, long long batch, hipStream_t stream) {
    const bool rows = a.bin_stride == 1;  // frame-major rows: lanes along the bins; anything else: lanes along time
    const int per = rows ? kTileF : kColsF;
    a.tiles_per_clip = (a.n_frames + per - 1) / per;
    if (a.tiles_per_clip * batch > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)(a.tiles_per_clip * batch));
    if (rows) hipLaunchKernelGGL(chroma_rows_kernel<T>, grid, dim3(kNT), 0, stream, a);
    else hipLaunchKernelGGL(chroma_cols_kernel<T>, grid, dim3(kNT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_chroma(Args a, long long batch, bool f64, hipStream_t stream) {
    if (batch <= 0 || a.n_frames <= 0 || a.n_chroma <= 0) return hipSuccess;
    return f64 ? launch_typed<double>(a, batch, stream) : launch_typed<float>(a, batch, stream);
}

}  // namespace chroma
}  // namespace lra

// ---- C entry points: chroma projection -----------------------------------------------------------------------------------------------------------
using namespace lra;

extern "C" {

int lra_chroma_exec(lra_ctx* ctx, const void* X, int64_t batch, int64_t n_bins, int64_t n_frames, int64_t batch_stride, int64_t bin_stride, int64_t frame_stride, int dtype,
                    const void* W, int64_t n_chroma, int norm, double threshold, int has_threshold, void* out, void* work, int* nonfinite) {
    LRA_BIND(ctx);
    if (nonfinite) *nonfinite = 0;
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "chroma: dtype must be LRA_F32 or LRA_F64");
    if (norm != LRA_CHROMA_NORM_NONE && norm != LRA_CHROMA_NORM_L1 && norm != LRA_CHROMA_NORM_L2 && norm != LRA_CHROMA_NORM_INF) return fail(LRA_EINVAL, "chroma: unknown norm");
    if (batch < 0 || n_bins < 0 || n_frames < 0 || n_chroma < 0) return fail(LRA_EINVAL, "chroma: negative size");
    if (batch == 0 || n_frames == 0 || n_chroma == 0) return LRA_OK;
    if (n_bins > 0x7fffffffLL || n_chroma > 0x7fffffffLL) return fail(LRA_EINVAL, "chroma: too many bins or rows");
    if ((n_bins > 0 && (!X || !W)) || !out || !work) return fail(LRA_EINVAL, "null data pointer");
    if (batch_stride < 0 || bin_stride < 0 || frame_stride < 0) return fail(LRA_EINVAL, "chroma: negative stride");
    chroma::Args a{};
    a.x = X;
    a.batch_stride = batch_stride;
    a.bin_stride = bin_stride;
    a.frame_stride = frame_stride;
    a.n_bins = (int)n_bins;
    a.n_frames = n_frames;
    a.w = W;
    a.n_chroma = (int)n_chroma;
    a.norm = norm;
    a.has_thr = has_threshold != 0;
    a.thr = threshold;
    a.out = out;
    a.flag = (int*)work;
    LRA_HIP(hipMemsetAsync(work, 0, sizeof(int), ctx->stream));
    LRA_HIP(chroma::launch_chroma(a, batch, dtype == LRA_F64, ctx->stream));
    if (nonfinite) {
        int h = 0;
        LRA_TRY(read_status(ctx, work, &h, sizeof(h)));
        *nonfinite = h != 0;
    }
    return LRA_OK;
}

}  // extern "C"
