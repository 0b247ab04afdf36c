// lra_pyin.h -- the back half of librosa.pyin that is not Viterbi (librosa/core/pitch.py:796-852, __pyin_helper :855-931): the observation
// table of every frame, written as the log table the decoder reads, and the lookup that turns the decoded states into f0.
// Self-contained so that tests/hostsim/pyinsim.cpp can run the same kernel bodies on host fibres (-DLRA_POSTSIM).
//
//   pyin_obs     cmnd, shifts [clip][lag][frame] float64 (what lra_yin_exec writes in LRA_YIN_FRAMES mode for float64 samples) ->
//                log_prob [clip][frame][2 P] float64 (lra_viterbi_exec's layout: viterbi_prep is skipped) and voiced_prob [clip][frame].
//                A wave per frame, g.waves frames per workgroup.  Per frame:
//                  troughs      util.localmin's rule on the lags, 64 at a time: c[i] < c[i - 1] and c[i] <= c[i + 1]; the last lag the first test
//                               alone; lag 0: c[0] < c[1].  A ballot gives the troughs of the 64 lags in lag order.
//                  thresholds   lane l owns the thresholds l, l + 64, ...  Pass 1 walks the troughs in lag order and counts N_j = #{h < t_j} per
//                               threshold (in LDS), and finds the first argmin of the heights.  Pass 2 walks them again with a running count k_ij
//                               per threshold: prob_i = sum_j (fact[N_j] E[k_ij]) beta_j, each lane over its own j ascending, the 64 partial sums
//                               joined by an xor butterfly (32, 16, .. 1): the order depends on n_thresholds alone.  fact[N] E[k] is scipy's
//                               boltzmann._pmf from the same two host tables, bit for bit.  The global minimum gets no_trough_prob *
//                               sum(beta[:n_below]) (a host table of prefix sums) added.
//                  binning      a trough with prob != 0: period = min_period + lag + shift, bin = clip(rint(12 nb log2(sr / period / fmin)), 0, P);
//                               the voiced row lives in LDS and lane 0 assigns row[bin] = prob in lag order (the reference's scatter is an
//                               assignment: the higher lag wins); bin P falls into the unvoiced block, which is overwritten: dropped.
//                  voiced_prob  the row's nonzero entries added in ascending bin order (adding the zeros between them changes nothing), clipped to
//                               [0, 1]; every unvoiced state gets the one value u = (1 - voiced_prob) / P.
//                  stored       log(p + tiny); p == 0 stores the host's log(tiny) constant; log(u + tiny) is computed once per frame.
//                No lane leaves before the end (every lane takes part in the ballots and the butterfly); a wave past the last frame works on the
//                last frame and stores nothing.
//   pyin_finish  states uint16 [n] -> f0 = freqs[state % P] (the host's float64 table), voiced = state < P (one byte), f0 = fill where not voiced.
#pragma once

#ifndef LRA_POSTSIM
#include <hip/hip_runtime.h>
#endif

#include <cstdint>

#ifdef LRA_POSTSIM
#define LRA_PYIN_DYN_LDS(ptr) char* ptr = reinterpret_cast<char*>(g_postsim_dyn_lds)
#else
#define LRA_PYIN_DYN_LDS(ptr) extern __shared__ __align__(16) char lra_pyin_lds[]; char* ptr = lra_pyin_lds
#endif

namespace lra {
namespace pyin {

constexpr int kLdsMax = 160 * 1024;
constexpr int kMaxWaves = 4;     // frames per workgroup, halved until the rows fit
constexpr int kFinishNT = 256;

// a wave's LDS: the voiced row (8 P bytes), N_j and the running count per threshold (4 bytes each)
constexpr long long wave_lds(int P, int n_thresholds) { return 8LL * P + 8LL * n_thresholds; }

struct Geometry {
    int waves;  // frames per workgroup
    int lds;    // bytes of dynamic LDS (above kLdsMax: refused)
};
constexpr Geometry geometry(int P, int n_thresholds) {
    Geometry g{};
    g.waves = kMaxWaves;
    while (g.waves > 1 && g.waves * wave_lds(P, n_thresholds) > kLdsMax) g.waves /= 2;
    const long long lds = g.waves * wave_lds(P, n_thresholds);
    g.lds = lds > 0x7fffffffLL ? 0x7fffffff : (int)lds;
    return g;
}

struct ObsArgs {
    const double* cmnd;         // [clip][lag][frame]
    const double* shifts;       // [clip][lag][frame]
    long long clips;
    int n_lags;                 // >= 2
    long long T;                // frames per clip
    const double* thresholds;   // [n_thresholds]: np.linspace(0, 1, n_thresholds + 1)[1:]
    const double* beta;         // [n_thresholds]: beta_probs
    const double* beta_prefix;  // [n_thresholds + 1]: np.sum(beta_probs[:m])
    const double* boltz_e;      // [n_lags + 1]: exp(-lambda k)
    const double* boltz_fact;   // [n_lags + 1]: (1 - exp(-lambda)) / (1 - exp(-lambda N))
    int n_thresholds;
    double sr, fmin;
    int min_period;
    int P;                      // n_pitch_bins
    int bins_per_octave;        // 12 * n_bins_per_semitone
    double no_trough_prob;
    double tiny, log_tiny;      // util.tiny of float64 and the host's log of it
    double* log_prob;           // [clip][frame][2 P]
    double* voiced_prob;        // [clip][frame]
    Geometry g;
};

struct FinishArgs {
    const uint16_t* states;  // [n]
    long long n;
    int P;
    const double* freqs;     // [P]
    int fill;                // write fill_na into unvoiced frames
    double fill_na;
    double* f0;              // [n]
    uint8_t* voiced;         // [n]
};

#ifdef LRA_POSTSIM
unsigned long long pyin_ballot(int pred);  // bit l: the predicate of lane l of my wave
double pyin_wave_sum(double v);            // the butterfly below, on every lane
int pyin_wave_sum(int v);
#else
__device__ __forceinline__ unsigned long long pyin_ballot(int pred) { return __ballot(pred); }
__device__ __forceinline__ double pyin_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ int pyin_wave_sum(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
#endif

// util.localmin with __pyin_helper's rule for lag 0 (:872-874); n >= 2
__device__ __forceinline__ bool pyin_is_trough(const double* c, long long stride, int i, int n) {
    const double x = c[(long long)i * stride];
    if (i == 0) return x < c[stride];
    const bool below_left = x < c[(long long)(i - 1) * stride];
    if (i == n - 1) return below_left;
    return below_left && x <= c[(long long)(i + 1) * stride];
}

// grid = ceil(clips * T / g.waves) workgroups of 64 g.waves threads; dynamic LDS = g.lds
__device__ __forceinline__ void obs_body(const ObsArgs& a) {
    LRA_PYIN_DYN_LDS(lds);
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int P = a.P, nthr = a.n_thresholds, n = a.n_lags;
    const long long total = a.clips * a.T;
    long long frame = (long long)blockIdx.x * a.g.waves + wave;
    const bool live = frame < total;
    if (!live) frame = total - 1;
    const long long clip = frame / a.T, t = frame % a.T;
    const long long stride = a.T;
    const double* c = a.cmnd + clip * n * stride + t;
    const double* sh = a.shifts + clip * n * stride + t;
    char* mine = lds + (long long)wave * wave_lds(P, nthr);
    double* row = reinterpret_cast<double*>(mine);
    int* count_all = reinterpret_cast<int*>(row + P);  // N_j
    int* count_run = count_all + nthr;                 // troughs below t_j met so far
    for (int j = lane; j < nthr; j += 64) {
        count_all[j] = 0;
        count_run[j] = 0;
    }
    for (int s = lane; s < P; s += 64) row[s] = 0.0;
    __syncthreads();

    // pass 1: N_j and the first argmin of the trough heights
    const double t_last = a.thresholds[nthr - 1];
    int n_troughs = 0, min_lag = -1;
    double min_h = 0.0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        unsigned long long votes = pyin_ballot(i < n && pyin_is_trough(c, stride, i, n));
        while (votes) {
            const int bit = __builtin_ctzll(votes);
            votes &= votes - 1;
            const double h = c[(long long)(base + bit) * stride];
            if (n_troughs == 0 || h < min_h) {
                min_h = h;
                min_lag = base + bit;
            }
            ++n_troughs;
            if (h < t_last)
                for (int j = lane; j < nthr; j += 64)
                    if (h < a.thresholds[j]) ++count_all[j];
        }
    }
    // what the global minimum gets besides: no_trough_prob * sum(beta[:n_below]), n_below = #{j: not (min_h < t_j)}
    double extra = 0.0;
    if (n_troughs > 0) {
        int below = 0;
        for (int j = lane; j < nthr; j += 64) below += !(min_h < a.thresholds[j]);
        extra = a.no_trough_prob * a.beta_prefix[pyin_wave_sum(below)];
    }

    // pass 2: the probability of every trough, assigned to its bin in lag order
    if (n_troughs > 0) {
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            unsigned long long votes = pyin_ballot(i < n && pyin_is_trough(c, stride, i, n));
            while (votes) {
                const int bit = __builtin_ctzll(votes);
                votes &= votes - 1;
                const int lag = base + bit;
                const double h = c[(long long)lag * stride];
                double prob = 0.0;
                if (h < t_last) {
                    double part = 0.0;
                    for (int j = lane; j < nthr; j += 64)
                        if (h < a.thresholds[j]) {
                            const int k = count_run[j]++;
                            part += (a.boltz_fact[count_all[j]] * a.boltz_e[k]) * a.beta[j];
                        }
                    prob = pyin_wave_sum(part);
                }
                if (lag == min_lag) prob += extra;
                if (prob != 0.0 && lane == 0) {
                    const double period = (double)(a.min_period + lag) + sh[(long long)lag * stride];
                    const double x = rint((double)a.bins_per_octave * log2(a.sr / period / a.fmin));
                    // np.clip(., 0, P): a NaN (never from finite audio) would be cast to an arbitrary integer there; it is dropped here
                    if (x < (double)P) row[x > 0.0 ? (int)x : 0] = prob;
                }
            }
        }
    }
    __syncthreads();

    // voiced_prob: the nonzero entries of the row in ascending bin order
    double voiced = 0.0;
    for (int base = 0; base < P; base += 64) {
        const int s = base + lane;
        unsigned long long votes = pyin_ballot(s < P && row[s] != 0.0);
        while (votes) {
            const int bit = __builtin_ctzll(votes);
            votes &= votes - 1;
            voiced += row[base + bit];
        }
    }
    voiced = voiced < 0.0 ? 0.0 : (voiced > 1.0 ? 1.0 : voiced);
    const double log_unvoiced = log((1.0 - voiced) / (double)P + a.tiny);
    if (live) {
        double* out = a.log_prob + frame * 2 * P;
        for (int s = lane; s < P; s += 64) {
            const double p = row[s];
            out[s] = p == 0.0 ? a.log_tiny : log(p + a.tiny);
            out[P + s] = log_unvoiced;
        }
        if (lane == 0) a.voiced_prob[frame] = voiced;
    }
}

// grid = ceil(n / kFinishNT) workgroups of kFinishNT threads
__device__ __forceinline__ void finish_body(const FinishArgs& a) {
    const long long at = (long long)blockIdx.x * kFinishNT + (long long)threadIdx.x;
    if (at >= a.n) return;
    const int s = a.states[at];
    const bool voiced = s < a.P;
    a.f0[at] = a.fill && !voiced ? a.fill_na : a.freqs[s % a.P];
    a.voiced[at] = voiced ? 1 : 0;
}

// (plain functions, not templates: defined where LRA_PYIN_KERNELS says so -- lra_pyin_inst.hip and the simulator -- and nowhere else)
#if defined(LRA_PYIN_KERNELS) || defined(LRA_POSTSIM)
__global__ __launch_bounds__(64 * kMaxWaves) void pyin_obs(ObsArgs a) { obs_body(a); }
__global__ __launch_bounds__(kFinishNT) void pyin_finish(FinishArgs a) { finish_body(a); }
#endif

}  // namespace pyin
}  // namespace lra
