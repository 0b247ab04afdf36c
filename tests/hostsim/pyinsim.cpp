// pyinsim.cpp -- runs the pYIN observation and finish kernel bodies of librosa_amd/csrc/lra_pyin.h on host fibres (tests/hostsim/simshim.h), with the
// launch geometry of the library's own host function (pyin::geometry).
//
// TEST INFRASTRUCTURE ONLY.  Built by tests/hostsim_util.py (sim_lib) into tests/hostsim/_pyinsim.so.
// Never linked into, imported by, or used as a fallback for the product library.
#define LRA_SIM_FIBRES 1
#include "simshim.h"

namespace lra {
namespace pyin {
unsigned long long pyin_ballot(int pred) { return sim::wave_ballot(pred); }
// the kernel's xor butterfly (32, 16, .. 1) over the 64 posted values; every lane ends with the same bits, lane 0's are taken
template <class T> static T butterfly(const T* s, unsigned me) {
    T v[64];
    const unsigned w0 = me & ~63u;
    for (unsigned l = 0; l < 64; ++l) v[l] = s[w0 + l];
    for (unsigned off = 32; off > 0; off >>= 1) {
        T next[64];
        for (unsigned l = 0; l < 64; ++l) next[l] = v[l] + v[l ^ off];
        for (unsigned l = 0; l < 64; ++l) v[l] = next[l];
    }
    return v[me & 63u];
}
double pyin_wave_sum(double v) { return sim::wave_exchange(v, [](const double* s, unsigned me) { return butterfly(s, me); }); }
int pyin_wave_sum(int v) { return sim::wave_exchange(v, [](const int* s, unsigned me) { return butterfly(s, me); }); }
}  // namespace pyin
}  // namespace lra

#include "../../librosa_amd/csrc/lra_pyin.h"

extern "C" {
// what lra_pyin_obs_exec decides for a size: out = {frames per workgroup, LDS bytes}
void pyinsim_geometry(int n_pitch_bins, int n_thresholds, int* out) {
    const lra::pyin::Geometry g = lra::pyin::geometry(n_pitch_bins, n_thresholds);
    out[0] = g.waves;
    out[1] = g.lds;
}

// the arguments of lra_pyin_obs_exec (include/librosa_amd.h), host pointers; returns -1 where the LDS does not fit
int pyinsim_obs(const double* cmnd, const double* shifts, long long clips, int n_lags, long long n_frames, const double* thresholds, const double* beta, const double* beta_prefix,
                const double* boltz_e, const double* boltz_fact, int n_thresholds, double sr, double fmin, int min_period, int n_pitch_bins, int n_bins_per_semitone, double no_trough_prob,
                double tiny, double log_tiny, double* log_prob, double* voiced_prob) {
    using namespace lra::pyin;
    if (wave_lds(n_pitch_bins, n_thresholds) > kLdsMax || n_lags < 2) return -1;
    ObsArgs a{};
    a.cmnd = cmnd;
    a.shifts = shifts;
    a.clips = clips;
    a.n_lags = n_lags;
    a.T = n_frames;
    a.thresholds = thresholds;
    a.beta = beta;
    a.beta_prefix = beta_prefix;
    a.boltz_e = boltz_e;
    a.boltz_fact = boltz_fact;
    a.n_thresholds = n_thresholds;
    a.sr = sr;
    a.fmin = fmin;
    a.min_period = min_period;
    a.P = n_pitch_bins;
    a.bins_per_octave = 12 * n_bins_per_semitone;
    a.no_trough_prob = no_trough_prob;
    a.tiny = tiny;
    a.log_tiny = log_tiny;
    a.log_prob = log_prob;
    a.voiced_prob = voiced_prob;
    a.g = geometry(n_pitch_bins, n_thresholds);
    if (clips <= 0 || n_frames <= 0) return 0;
    run_grid((unsigned)((clips * n_frames + a.g.waves - 1) / a.g.waves), 64u * (unsigned)a.g.waves, [=] { pyin_obs(a); });
    return 0;
}

// the arguments of lra_pyin_finish_exec, host pointers
int pyinsim_finish(const uint16_t* states, long long n, int n_pitch_bins, const double* freqs, int fill, double fill_na, double* f0, uint8_t* voiced) {
    using namespace lra::pyin;
    FinishArgs a{states, n, n_pitch_bins, freqs, fill != 0, fill_na, f0, voiced};
    if (n <= 0) return 0;
    run_grid_serial((unsigned)((n + kFinishNT - 1) / kFinishNT), kFinishNT, [=] { pyin_finish(a); });
    return 0;
}
}
