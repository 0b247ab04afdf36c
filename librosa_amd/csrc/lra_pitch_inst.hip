// lra_pitch_inst.hip -- instances and the launchers of the pitch kernels (lra_pitch.h) and the C entry points they serve, a translation unit of its
// own so that it compiles side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#include "lra_pitch.h"

#include "lra_internal.h"

namespace lra {
namespace pitch {

static unsigned stride_grid(long long n_segments) {
    const long long want = (n_segments + kWaves - 1) / kWaves;
    return (unsigned)(want < 1 ? 1 : (want > kMaxGrid ? kMaxGrid : want));
}

template <class T, bool kEmit> static hipError_t launch_typed(Args a, long long batch, hipStream_t stream) {
    const bool rows = a.bin_stride == 1 && (kEmit || a.out_bin_stride == 1);  // frame-major rows: lanes along the bins; anything else: lanes along time
    const int per = rows ? kRowsF : kColsF;
    a.tiles_per_clip = (a.n_frames + per - 1) / per;
    if (a.tiles_per_clip * batch > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)(a.tiles_per_clip * batch));
    if (rows) hipLaunchKernelGGL((piptrack_rows_kernel<T, kEmit>), grid, dim3(kNT), 0, stream, a);
    else hipLaunchKernelGGL((piptrack_cols_kernel<T, kEmit>), grid, dim3(kNT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_piptrack(Args a, long long batch, bool emit, bool f64, hipStream_t stream) {
    if (batch <= 0 || a.n_frames <= 0 || a.n_bins <= 0) return hipSuccess;
    if (emit) return f64 ? launch_typed<double, true>(a, batch, stream) : launch_typed<float, true>(a, batch, stream);
    return f64 ? launch_typed<double, false>(a, batch, stream) : launch_typed<float, false>(a, batch, stream);
}

template <class T> static hipError_t median_typed(SelectArgs a, hipStream_t stream) {
    const dim3 grid(stride_grid(a.n_segments));
    for (int pass = 0; pass < Passes<T>::value; ++pass) {
        hipLaunchKernelGGL(select_count_kernel<T>, grid, dim3(kNT), 0, stream, a, pass);
        hipLaunchKernelGGL(select_scan_kernel<T>, dim3(1), dim3(kNT), 0, stream, a, pass);
    }
    return hipGetLastError();
}

hipError_t launch_median(SelectArgs a, bool f64, hipStream_t stream) { return f64 ? median_typed<double>(a, stream) : median_typed<float>(a, stream); }

hipError_t launch_tuning_hist(HistArgs a, bool f64, hipStream_t stream) {
    if (a.n_segments <= 0) return hipSuccess;
    const dim3 grid(stride_grid(a.n_segments));
    if (f64) hipLaunchKernelGGL(tuning_hist_kernel<double>, grid, dim3(kNT), 0, stream, a);
    else hipLaunchKernelGGL(tuning_hist_kernel<float>, grid, dim3(kNT), 0, stream, a);
    return hipGetLastError();
}

}  // namespace pitch
}  // namespace lra

// ---- C entry points: pitch tracking and tuning ---------------------------------------------------------------------------------------------------
using namespace lra;

extern "C" {

static_assert(pitch::kRefMax == LRA_PITCH_REF_MAX && pitch::kRefRow == LRA_PITCH_REF_ROW && pitch::kRefScalar == LRA_PITCH_REF_SCALAR, "pitch ref codes");

namespace {
struct TuningWork {
    int64_t state, hist, count, peak_pitch, peak_mag, total;
    int cap;
};
TuningWork tuning_work_layout(int64_t batch, int64_t n_frames, int64_t masked_bins, int dtype) {
    auto up = [](int64_t b) { return (b + 255) / 256 * 256; };
    const int64_t frames = (batch > 0 ? batch : 0) * (n_frames > 0 ? n_frames : 0);
    const int64_t es = dtype == LRA_F64 ? 8 : 4;
    TuningWork w{};
    w.cap = (int)(((masked_bins > 1 ? masked_bins : 1) + 1) / 2);
    w.state = 0;
    w.hist = 256;
    w.count = w.hist + up(2 * pitch::kDigits * 8);
    w.peak_pitch = w.count + up(frames * 4);
    w.peak_mag = w.peak_pitch + up(frames * w.cap * es);
    w.total = w.peak_mag + up(frames * w.cap * es);
    return w;
}

// the checks lra_piptrack_exec and lra_tuning_exec share; fills what both kernels' forms read
int pitch_args(pitch::Args& a, const void* S, int64_t batch, int64_t n_bins, int64_t n_frames, int64_t batch_stride, int64_t bin_stride, int64_t frame_stride, int dtype, int64_t bin_lo,
               int64_t bin_hi, int ref_mode, double threshold, const void* ref_row, double ref_scalar, double sr, int64_t n_fft) {
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "piptrack: dtype must be LRA_F32 or LRA_F64");
    if (ref_mode != LRA_PITCH_REF_MAX && ref_mode != LRA_PITCH_REF_ROW && ref_mode != LRA_PITCH_REF_SCALAR) return fail(LRA_EINVAL, "piptrack: unknown ref mode");
    if (batch < 0 || n_bins < 0 || n_frames < 0) return fail(LRA_EINVAL, "piptrack: negative size");
    if (n_bins > 0x7fffffffLL - 64) return fail(LRA_EINVAL, "piptrack: too many bins");
    if (batch_stride < 0 || bin_stride < 0 || frame_stride < 0) return fail(LRA_EINVAL, "piptrack: negative stride");
    if (n_fft <= 0) return fail(LRA_EINVAL, "piptrack: n_fft must be positive");
    if (batch > 0 && n_bins > 0 && n_frames > 0 && (!S || (ref_mode == LRA_PITCH_REF_ROW && !ref_row))) return fail(LRA_EINVAL, "null data pointer");
    a.s = S;
    a.batch_stride = batch_stride;
    a.bin_stride = bin_stride;
    a.frame_stride = frame_stride;
    a.n_bins = (int)n_bins;
    a.n_frames = n_frames;
    a.lo = (int)(bin_lo < 0 ? 0 : (bin_lo > n_bins ? n_bins : bin_lo));
    a.hi = (int)(bin_hi < 0 ? 0 : (bin_hi > n_bins ? n_bins : bin_hi));
    a.ref_mode = ref_mode;
    a.threshold = threshold;
    a.ref_row = (const double*)ref_row;
    a.ref_scalar = ref_scalar;
    a.sr = sr;
    a.n_fft = (double)n_fft;
    return LRA_OK;
}
}  // namespace

int lra_piptrack_exec(lra_ctx* ctx, const void* S, int64_t batch, int64_t n_bins, int64_t n_frames, int64_t batch_stride, int64_t bin_stride, int64_t frame_stride, int dtype,
                      int64_t bin_lo, int64_t bin_hi, int ref_mode, double threshold, const void* ref_row, double ref_scalar, double sr, int64_t n_fft, void* pitches, void* mags,
                      int64_t out_batch_stride, int64_t out_bin_stride, int64_t out_frame_stride) {
    LRA_BIND(ctx);
    pitch::Args a{};
    const int rc = pitch_args(a, S, batch, n_bins, n_frames, batch_stride, bin_stride, frame_stride, dtype, bin_lo, bin_hi, ref_mode, threshold, ref_row, ref_scalar, sr, n_fft);
    if (rc != LRA_OK) return rc;
    if (batch == 0 || n_bins == 0 || n_frames == 0) return LRA_OK;
    if (!pitches || !mags) return fail(LRA_EINVAL, "null data pointer");
    if (out_batch_stride < 0 || out_bin_stride < 0 || out_frame_stride < 0) return fail(LRA_EINVAL, "piptrack: negative stride");
    a.pitches = pitches;
    a.mags = mags;
    a.out_batch_stride = out_batch_stride;
    a.out_bin_stride = out_bin_stride;
    a.out_frame_stride = out_frame_stride;
    LRA_HIP(pitch::launch_piptrack(a, batch, false, dtype == LRA_F64, ctx->stream));
    return LRA_OK;
}

int64_t lra_tuning_work_bytes(int64_t batch, int64_t n_frames, int64_t masked_bins, int dtype) { return tuning_work_layout(batch, n_frames, masked_bins, dtype).total; }

int lra_tuning_exec(lra_ctx* ctx, const void* S, int64_t batch, int64_t n_bins, int64_t n_frames, int64_t batch_stride, int64_t bin_stride, int64_t frame_stride, int dtype,
                    int64_t bin_lo, int64_t bin_hi, int ref_mode, double threshold, const void* ref_row, double ref_scalar, double sr, int64_t n_fft, const void* edges, int64_t n_hist,
                    double bins_per_octave, void* work, void* out) {
    LRA_BIND(ctx);
    pitch::Args a{};
    const int rc = pitch_args(a, S, batch, n_bins, n_frames, batch_stride, bin_stride, frame_stride, dtype, bin_lo, bin_hi, ref_mode, threshold, ref_row, ref_scalar, sr, n_fft);
    if (rc != LRA_OK) return rc;
    if (n_hist <= 0 || n_hist > 0x7fffffffLL - 2) return fail(LRA_EINVAL, "tuning: the histogram needs between 1 and 2^31 - 3 bins");
    if (!edges || !work || !out) return fail(LRA_EINVAL, "null data pointer");
    const TuningWork w = tuning_work_layout(batch, n_frames, a.hi - a.lo, dtype);
    char* base = (char*)work;
    LRA_HIP(hipMemsetAsync(out, 0, (size_t)(n_hist + 2) * 8, ctx->stream));
    if (batch == 0 || n_bins == 0 || n_frames == 0) return LRA_OK;
    LRA_HIP(hipMemsetAsync(work, 0, (size_t)w.count, ctx->stream));  // the select's state and histogram
    a.peak_pitch = base + w.peak_pitch;
    a.peak_mag = base + w.peak_mag;
    a.peak_count = (int*)(base + w.count);
    a.cap = w.cap;
    const bool f64 = dtype == LRA_F64;
    LRA_HIP(pitch::launch_piptrack(a, batch, true, f64, ctx->stream));
    pitch::SelectState* state = (pitch::SelectState*)(base + w.state);
    pitch::SelectArgs sel{a.peak_mag, a.peak_count, batch * n_frames, w.cap, (unsigned long long*)(base + w.hist), state};
    LRA_HIP(pitch::launch_median(sel, f64, ctx->stream));
    pitch::HistArgs h{a.peak_pitch, a.peak_mag, a.peak_count, batch * n_frames, batch * n_frames * w.cap, w.cap, state, (const double*)edges, (int)n_hist, bins_per_octave,
                      (unsigned long long*)out};
    LRA_HIP(pitch::launch_tuning_hist(h, f64, ctx->stream));
    LRA_HIP(hipMemcpyAsync((char*)out + (size_t)(n_hist + 1) * 8, &state->total, 8, hipMemcpyDeviceToDevice, ctx->stream));
    return LRA_OK;
}

int lra_pitch_tuning_exec(lra_ctx* ctx, const void* freq, int64_t n, int dtype, const void* edges, int64_t n_hist, double bins_per_octave, void* out) {
    LRA_BIND(ctx);
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "pitch_tuning: dtype must be LRA_F32 or LRA_F64");
    if (n < 0) return fail(LRA_EINVAL, "pitch_tuning: negative size");
    if (n_hist <= 0 || n_hist > 0x7fffffffLL - 2) return fail(LRA_EINVAL, "pitch_tuning: the histogram needs between 1 and 2^31 - 3 bins");
    if (!edges || !out || (n > 0 && !freq)) return fail(LRA_EINVAL, "null data pointer");
    LRA_HIP(hipMemsetAsync(out, 0, (size_t)(n_hist + 2) * 8, ctx->stream));
    const int64_t n_segments = (n + pitch::kPlainSeg - 1) / pitch::kPlainSeg;
    pitch::HistArgs h{freq, nullptr, nullptr, n_segments, n, pitch::kPlainSeg, nullptr, (const double*)edges, (int)n_hist, bins_per_octave, (unsigned long long*)out};
    LRA_HIP(pitch::launch_tuning_hist(h, dtype == LRA_F64, ctx->stream));
    return LRA_OK;
}

}  // extern "C"
