// lra_pyin_inst.hip -- the pYIN observation and finish kernels (lra_pyin.h) and their launchers and the C entry points they serve, a translation unit
// of its own so that it compiles side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#define LRA_PYIN_KERNELS 1
#include "lra_pyin.h"

#include "lra_internal.h"

namespace lra {
namespace pyin {

hipError_t launch_obs(const ObsArgs& a, hipStream_t stream) {
    if (a.clips <= 0 || a.T <= 0) return hipSuccess;
    const Geometry& g = a.g;
    if (g.lds > kLdsMax || g.waves < 1 || g.waves > kMaxWaves) return hipErrorInvalidConfiguration;
    const long long grid = (a.clips * a.T + g.waves - 1) / g.waves;
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    if (g.lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pyin_obs), hipFuncAttributeMaxDynamicSharedMemorySize, g.lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(pyin_obs, dim3((unsigned)grid), dim3(64 * g.waves), g.lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_finish(const FinishArgs& a, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    const long long grid = (a.n + kFinishNT - 1) / kFinishNT;
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(pyin_finish, dim3((unsigned)grid), dim3(kFinishNT), 0, stream, a);
    return hipGetLastError();
}

}  // namespace pyin
}  // namespace lra

// ---- C entry points: the back half of pyin around the decode -------------------------------------------------------------------------------------
using namespace lra;

extern "C" {

static_assert(pyin::kLdsMax == LRA_PYIN_LDS_MAX, "pyin limits");
static_assert(pyin::geometry(601, 100).waves == 4 && pyin::geometry(4096, 100).lds <= pyin::kLdsMax, "pyin: the default call and the largest state count fit");

int64_t lra_pyin_lds_bytes(int n_pitch_bins, int n_thresholds) {
    if (n_pitch_bins < 1 || n_thresholds < 1) return 0;
    const pyin::Geometry g = pyin::geometry(n_pitch_bins, n_thresholds);
    return g.waves > 1 ? (int64_t)g.lds : (int64_t)pyin::wave_lds(n_pitch_bins, n_thresholds);
}

int lra_pyin_obs_exec(lra_ctx* ctx, const void* cmnd, const void* shifts, int64_t clips, int n_lags, int64_t n_frames, const void* thresholds, const void* beta_probs,
                      const void* beta_prefix, const void* boltz_e, const void* boltz_fact, int n_thresholds, double sr, double fmin, int min_period, int n_pitch_bins,
                      int n_bins_per_semitone, double no_trough_prob, double tiny, double log_tiny, void* log_prob, void* voiced_prob) {
    LRA_BIND(ctx);
    if (clips < 0 || n_frames < 0 || n_lags < 2) return fail(LRA_EINVAL, "pyin: need at least 2 lags and non-negative sizes");
    if (n_thresholds < 1 || n_pitch_bins < 1 || n_bins_per_semitone < 1 || min_period < 1) return fail(LRA_EINVAL, "pyin: n_thresholds, n_pitch_bins, n_bins_per_semitone and min_period must be positive");
    if (12LL * n_bins_per_semitone > 0x7fffffffLL) return fail(LRA_EINVAL, "pyin: n_bins_per_semitone is too large");
    if (!(sr > 0) || !(fmin > 0)) return fail(LRA_EINVAL, "pyin: sr and fmin must be positive");
    if (pyin::wave_lds(n_pitch_bins, n_thresholds) > pyin::kLdsMax)
        return fail(LRA_EINVAL, "pyin: n_pitch_bins=" + std::to_string(n_pitch_bins) + " with n_thresholds=" + std::to_string(n_thresholds) + " does not fit the LDS of a workgroup");
    if (clips == 0 || n_frames == 0) return LRA_OK;
    if (!cmnd || !shifts || !thresholds || !beta_probs || !beta_prefix || !boltz_e || !boltz_fact || !log_prob || !voiced_prob) return fail(LRA_EINVAL, "null data pointer");
    pyin::ObsArgs a{};
    a.cmnd = (const double*)cmnd;
    a.shifts = (const double*)shifts;
    a.clips = clips;
    a.n_lags = n_lags;
    a.T = n_frames;
    a.thresholds = (const double*)thresholds;
    a.beta = (const double*)beta_probs;
    a.beta_prefix = (const double*)beta_prefix;
    a.boltz_e = (const double*)boltz_e;
    a.boltz_fact = (const double*)boltz_fact;
    a.n_thresholds = n_thresholds;
    a.sr = sr;
    a.fmin = fmin;
    a.min_period = min_period;
    a.P = n_pitch_bins;
    a.bins_per_octave = 12 * n_bins_per_semitone;
    a.no_trough_prob = no_trough_prob;
    a.tiny = tiny;
    a.log_tiny = log_tiny;
    a.log_prob = (double*)log_prob;
    a.voiced_prob = (double*)voiced_prob;
    a.g = pyin::geometry(n_pitch_bins, n_thresholds);
    LRA_HIP(pyin::launch_obs(a, ctx->stream));
    return LRA_OK;
}

int lra_pyin_finish_exec(lra_ctx* ctx, const void* states, int64_t n, int n_pitch_bins, const void* freqs, int fill, double fill_na, void* f0, void* voiced_flag) {
    LRA_BIND(ctx);
    if (n < 0 || n_pitch_bins < 1) return fail(LRA_EINVAL, "pyin: negative size");
    if (n == 0) return LRA_OK;
    if (!states || !freqs || !f0 || !voiced_flag) return fail(LRA_EINVAL, "null data pointer");
    pyin::FinishArgs a{};
    a.states = (const uint16_t*)states;
    a.n = n;
    a.P = n_pitch_bins;
    a.freqs = (const double*)freqs;
    a.fill = fill != 0;
    a.fill_na = fill_na;
    a.f0 = (double*)f0;
    a.voiced = (uint8_t*)voiced_flag;
    LRA_HIP(pyin::launch_finish(a, ctx->stream));
    return LRA_OK;
}

}  // extern "C"
