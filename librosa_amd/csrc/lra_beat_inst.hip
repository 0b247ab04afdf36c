// lra_beat_inst.hip -- instances and the launcher of the beat-tracker kernels (lra_beat.h) and the C entry points they serve, a translation unit of
// its own so that it compiles side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#include "lra_beat.h"

#include "lra_internal.h"

namespace lra {
namespace beat {

template <class T> static hipError_t launch_typed(const Args& a, long long batch, hipStream_t stream) {
    const long long blocks = (a.n + 255) / 256;
    if (batch > 0x7fffffffLL || blocks * batch > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(beat_prepare_kernel<T>, dim3((unsigned)batch), dim3(kBeatPrepNT), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(beat_local_score_kernel<T>, dim3((unsigned)(blocks * batch)), dim3(256), 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(beat_track_kernel<T>, dim3((unsigned)batch), dim3(kBeatWave), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_beat(const Args& a, long long batch, bool f64, hipStream_t stream) {
    if (batch <= 0 || a.n <= 0) return hipSuccess;
    return f64 ? launch_typed<double>(a, batch, stream) : launch_typed<float>(a, batch, stream);
}

}  // namespace beat
}  // namespace lra

// ---- C entry points: beat tracker ----------------------------------------------------------------------------------------------------------------
using namespace lra;

extern "C" {

static_assert(beat::kPerRow == LRA_BEAT_BPM_PER_ROW && beat::kPerFrame == LRA_BEAT_BPM_PER_FRAME, "beat codes");

namespace {
struct BeatWork {
    int64_t any, dead, fpb, norm, local, cum, backlink, order, total;
};
BeatWork beat_work_layout(int64_t batch, int64_t n, int bpm_mode) {
    auto up = [](int64_t b) { return (b + 255) / 256 * 256; };
    const int64_t rows = batch > 0 ? batch : 0, cells = rows * (n > 0 ? n : 0);
    BeatWork w{};
    w.any = 0;
    w.dead = 256;
    w.fpb = w.dead + up(rows * 4);
    w.norm = w.fpb + up((bpm_mode == LRA_BEAT_BPM_PER_FRAME ? cells : rows) * 8);
    w.local = w.norm + up(cells * 8);
    w.cum = w.local + up(cells * 8);
    w.backlink = w.cum + up(cells * 8);
    w.order = w.backlink + up(cells * 4);
    w.total = w.order + up(cells * 4);
    return w;
}
}  // namespace

int64_t lra_beat_work_bytes(int64_t batch, int64_t n, int bpm_mode) { return beat_work_layout(batch, n, bpm_mode).total; }

int lra_beat_exec(lra_ctx* ctx, const void* env, int64_t batch, int64_t n, int dtype, const void* bpm, int bpm_mode, double frame_rate, double tightness, int trim, void* out,
                  void* work, int* any_nonzero) {
    LRA_BIND(ctx);
    if (any_nonzero) *any_nonzero = 0;
    if (bpm_mode != LRA_BEAT_BPM_PER_ROW && bpm_mode != LRA_BEAT_BPM_PER_FRAME) return fail(LRA_EINVAL, "beat: unknown bpm mode");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "beat: dtype must be LRA_F32 or LRA_F64");
    if (batch < 0 || n < 0) return fail(LRA_EINVAL, "beat: negative size");
    if (!(tightness > 0)) return fail(LRA_EINVAL, "beat: tightness must be strictly positive");
    if (!(frame_rate > 0)) return fail(LRA_EINVAL, "beat: frame_rate must be strictly positive");
    if (batch == 0 || n == 0) return LRA_OK;
    if (!env || !bpm || !out || !work) return fail(LRA_EINVAL, "null data pointer");
    if (n > 0x7fffffffLL) return fail(LRA_EINVAL, "beat: too many frames per row");
    const BeatWork w = beat_work_layout(batch, n, bpm_mode);
    char* base = (char*)work;
    beat::Args a{};
    a.env = env;
    a.n = n;
    a.bpm = (const double*)bpm;
    a.bpm_mode = bpm_mode;
    a.frame_rate = frame_rate;
    a.tightness = (float)tightness;
    a.trim = trim != 0;
    a.any = (int*)(base + w.any);
    a.dead = (int*)(base + w.dead);
    a.fpb = (double*)(base + w.fpb);
    a.norm = base + w.norm;
    a.local = base + w.local;
    a.cum = (double*)(base + w.cum);
    a.backlink = (int*)(base + w.backlink);
    a.order = (int*)(base + w.order);
    a.out = (unsigned char*)out;
    LRA_HIP(hipMemsetAsync(work, 0, sizeof(int), ctx->stream));
    LRA_HIP(beat::launch_beat(a, batch, dtype == LRA_F64, ctx->stream));
    if (any_nonzero) {
        int h = 0;
        LRA_TRY(read_status(ctx, work, &h, sizeof(int)));
        *any_nonzero = h != 0;
    }
    return LRA_OK;
}

}  // extern "C"
