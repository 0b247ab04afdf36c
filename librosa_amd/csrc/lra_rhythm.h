// lra_rhythm.h -- the autocorrelation tempogram and the tempo estimate: librosa.feature.tempogram / tempo
// (librosa/feature/rhythm.py:38-191, 295-471; autocorrelate: librosa/core/audio.py:1320-1394; util.normalize: util/utils.py:797-1020).
// Self-contained so that tests/hostsim/rhythmsim.cpp can run the same kernel bodies on host threads (-DLRA_POSTSIM).
//
//   padded  = np.pad(env, W // 2, mode="linear_ramp", end_values=0)     (centre; the ramp is folded into the load index, see rhythm_sample)
//   frame t = padded[t : t + W] * window                                 (float64 from here on, whatever the envelope's type)
//   r_t[m]  = irfft(|rfft(frame t, n=N)|^2)[m],  m < W                   (N >= 2 W - 1: zero padding makes the circular correlation linear)
//   col t   = r_t / length_t, length_t = max |r_t| | sum |r_t| | sqrt(sum r_t^2) | 1, set to 1 below tiny (normalize, fill=None)
//
// A workgroup of 256 threads owns kRhythmGroup consecutive frames of one clip and transforms them chunk_frames<N>() at a time with the Stockham
// passes and twiddle tables of lra::mixed (lra_mixed.h): the window-multiplied frame packed as N / 2 complex points, the forward passes,
// then ONE stage that does the Hermitian split, |X|^2 and the Hermitian un-split of the inverse (both touch the same bin pair (k, M - k)),
// then the forward passes again on the conjugate (FFT(conj Z') = conj of M times the inverse).  Everything after the load is float64.
// Window lengths whose 2 W - 1 exceeds the largest size of the list take tempogram_kernel<0>: the same epilogues over an O(W^2) sum.
//
// Three epilogues, chosen at run time:
//   WRITE   the normalised [clip][lag][frame] float64 tempogram.  The group's columns are staged in LDS as a [W][kRhythmGroup] tile and
//           written lag row by lag row (16 frames = 128 bytes per row) when the tile fits the LDS, else column by column.
//   SUM     per-group sums of the normalised columns, frame after frame ([clip][group][W]); tempo_mean_finish_kernel adds the groups in
//           order, divides by n_frames (np.mean), scores log1p(1e6 mean) + logprior and takes np.argmax's index.  The order of every
//           addition depends on the frame index alone, so a clip gives the same bits alone and inside a batch.
//   ARGMAX  per frame: log1p(1e6 col) + logprior, np.argmax, bpms[index] -- one float64 per frame.
// A column that is not finite sets *flag (the reference's normalize raises "Input must be finite" for every norm, None included).
#pragma once

#ifndef LRA_POSTSIM
#include <hip/hip_runtime.h>
#endif

#include "lra_mixed.h"
#include "lra_mixed_sizes.h"

#ifdef LRA_POSTSIM
#define LRA_RHYTHM_DYN_LDS(ptr) char* ptr = reinterpret_cast<char*>(g_postsim_dyn_lds)
#else
#define LRA_RHYTHM_DYN_LDS(ptr) extern __shared__ __align__(16) char lra_rhythm_lds[]; char* ptr = lra_rhythm_lds
#endif

namespace lra {
namespace rhythm {

using mixed::cpx;
using mixed::fma_t;
using mixed::mkc;

// modes and norms (the LRA_TEMPOGRAM_* values of include/librosa_amd.h)
constexpr int kWrite = 0, kSum = 1, kArgmax = 2;
constexpr int kNormNone = 0, kNormInf = 1, kNormL1 = 2, kNormL2 = 3;
constexpr int kRhythmNT = mixed::NT;  // threads per workgroup (the passes deal their work items over this many)
constexpr int kRhythmGroup = 16;      // frames per workgroup: 16 float64 = one 128-byte run of a lag row
constexpr int kRhythmRed = 64;        // lanes per frame in the column reductions
constexpr int kRhythmLdsMax = 160 * 1024;
constexpr double kRhythmTiny = 2.2250738585072014e-308;  // np.finfo(np.float64).tiny: util.tiny of the float64 autocorrelation

// frames transformed at a time: two ping-pong buffers of N / 2 complex doubles per frame within 48 KB (a power of two dividing the group)
constexpr int chunk_frames_of(int N) {
    int fc = kRhythmGroup;
    while (fc > 1 && fc * 2 * (N / 2) * 16 > 48 * 1024) fc /= 2;
    return fc;
}
template <int N> constexpr int chunk_frames() { return chunk_frames_of(N); }

// LDS layout (bytes, host and device): [FFT buffers + W_M table | direct: frame + r row] [reduction values][reduction indices][lengths]
// [SUM: W running sums | WRITE with tile: W x kRhythmGroup]
struct Lds {
    int core, red, redi, len, extra, total;
};
constexpr Lds lds_layout(int N, int W, int mode, bool tile) {
    Lds l{};
    const int fc = N > 0 ? chunk_frames_of(N) : 1;
    l.core = N > 0 ? (2 * fc * (N / 2) + N / 2) * 16 : 2 * W * 8;
    l.red = l.core;
    l.redi = l.red + fc * kRhythmRed * 8;
    l.len = l.redi + fc * kRhythmRed * 4;
    l.extra = l.len + fc * 8;
    l.total = l.extra + (mode == kSum ? W * 8 : (mode == kWrite && tile ? W * kRhythmGroup * 8 : 0));
    return l;
}

struct Args {
    const void* env;         // [batch][n] float32 or float64 (env_f64)
    int env_f64;
    long long n;             // envelope frames
    long long n_frames;      // tempogram frames: n (centre) or n - W + 1
    int W, pad;              // pad = W / 2 (centre) or 0
    int N;                   // transform length (0: direct kernel)
    const double* win;       // [W] float64 window
    const cpx<double>* tw_m; // [N / 2]     W_M^t
    const cpx<double>* tw_n; // [N / 2 + 1] W_N^k
    int norm, mode, tile;
    const double* logprior;  // [W] (SUM / ARGMAX)
    const double* bpms;      // [W] (ARGMAX)
    double* out;             // WRITE [batch][W][n_frames]; ARGMAX [batch][n_frames]
    double* partial;         // SUM [batch][groups][W]
    int* flag;               // set to 1 where a column is not finite
    int groups;              // ceil(n_frames / kRhythmGroup)
};

// the smallest size of LRA_MIXED_SIZES that holds the linear autocorrelation of W samples (2 W - 1), or 0: the direct kernel
constexpr int transform_length(int W) { return mixed::smallest_size_at_least(2 * W - 1); }

// Host: the geometry of one lra_tempogram_exec call, from its scalar parameters into a (the pointers and env_f64 stay the caller's).  Answers
// mixed::kGeometryTooShort (only W and pad set: the padded envelope does not hold one frame) or, everything set, mixed::kGeometryLds (no kernel fits
// the LDS of a workgroup for this W).  direct: the O(W^2) kernel whatever the size list offers -- the host simulator's switch.
inline int prepare(Args& a, long long n, int W, int center, int norm, int mode, bool direct = false) {
    a.W = W;
    a.pad = center ? W / 2 : 0;
    if (n + 2 * (long long)a.pad < W) return mixed::kGeometryTooShort;
    a.n = n;
    a.n_frames = center ? n : n - W + 1;
    a.N = direct ? 0 : transform_length(W);
    a.norm = norm;
    a.mode = mode;
    a.tile = mode == kWrite && lds_layout(a.N, W, mode, true).total <= kRhythmLdsMax;
    a.groups = (int)((a.n_frames + kRhythmGroup - 1) / kRhythmGroup);
    return lds_layout(a.N, W, mode, false).total > kRhythmLdsMax ? mixed::kGeometryLds : mixed::kGeometryOk;
}

// padded position q of a clip: np.pad(mode="linear_ramp", end_values=0) builds each ramp with np.linspace(0, edge, pad, endpoint=False)
// in float64 -- i * (edge / pad) -- and rounds it once to the envelope's dtype; the right ramp is the reversed one
__device__ __forceinline__ double rhythm_load(const Args& a, long long at) {
    return a.env_f64 ? reinterpret_cast<const double*>(a.env)[at] : (double)reinterpret_cast<const float*>(a.env)[at];
}
__device__ __forceinline__ double rhythm_sample(const Args& a, long long clip, long long q) {
    const long long e = q - a.pad, base = clip * a.n;
    if (e >= 0 && e < a.n) return rhythm_load(a, base + e);
    const long long i = e < 0 ? q : a.pad - 1 - (e - a.n);
    const double edge = rhythm_load(a, base + (e < 0 ? 0 : a.n - 1));
    const double v = (double)i * (edge / (double)a.pad) + 0.0;
    return a.env_f64 ? v : (double)(float)v;
}

// np.argmax's order: the first NaN wins; otherwise the larger value, the lower index on a tie; bi < 0: nothing taken yet
__device__ __forceinline__ bool rhythm_better(double v, int i, double bv, int bi) {
    if (bi < 0) return true;
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

__device__ __forceinline__ double rhythm_score(double v, double logprior) { return log1p(1e6 * v) + logprior; }

// The epilogue of one chunk: R holds `frames` autocorrelation rows (lags 0 .. W - 1, row pitch ld doubles) of group frames c0 .. c0 + frames - 1.
// Ends with a barrier: R may be overwritten afterwards.
__device__ __forceinline__ void rhythm_epilogue(const Args& a, char* lds, const Lds& L, const double* R, int ld, int frames, long long clip, int group, int c0) {
    double* red = reinterpret_cast<double*>(lds + L.red);
    int* redi = reinterpret_cast<int*>(lds + L.redi);
    double* len = reinterpret_cast<double*>(lds + L.len);
    double* extra = reinterpret_cast<double*>(lds + L.extra);
    const int tid = (int)threadIdx.x, W = a.W;
    const long long t0 = (long long)group * kRhythmGroup + c0;  // clip frame of R's first row
    // (1) column reductions: 64 lanes per frame over lags l, l + 64, ...; the finiteness test of util.normalize on the way
    for (int w = tid; w < frames * kRhythmRed; w += kRhythmNT) {
        const int f = w / kRhythmRed, l = w - f * kRhythmRed;
        double acc = 0.0;
        bool bad = false;
        for (int m = l; m < W; m += kRhythmRed) {
            const double v = R[f * ld + m], av = v < 0 ? -v : v;
            bad |= !(av <= 1.79769313486231570815e308);
            if (a.norm == kNormInf) acc = av > acc ? av : acc;
            else if (a.norm == kNormL1) acc += av;
            else if (a.norm == kNormL2) acc = fma_t(av, av, acc);
        }
        if (bad) *a.flag = 1;
        red[w] = acc;
    }
    __syncthreads();
    for (int f = tid; f < frames; f += kRhythmNT) {
        double acc = red[f * kRhythmRed];
        for (int l = 1; l < kRhythmRed; ++l) {
            const double v = red[f * kRhythmRed + l];
            if (a.norm == kNormInf) acc = v > acc ? v : acc;
            else acc += v;
        }
        if (a.norm == kNormL2) acc = sqrt(acc);
        if (a.norm == kNormNone || acc < kRhythmTiny) acc = 1.0;  // fill=None: a column below the threshold stays as it is
        len[f] = acc;
    }
    __syncthreads();
    if (a.mode == kWrite) {
        for (int f = 0; f < frames; ++f) {
            const double d = len[f];
            for (int m = tid; m < W; m += kRhythmNT) {
                const double v = R[f * ld + m] / d;
                if (a.tile) extra[m * kRhythmGroup + c0 + f] = v;
                else a.out[(clip * W + m) * a.n_frames + t0 + f] = v;
            }
        }
    } else if (a.mode == kSum) {
        for (int m = tid; m < W; m += kRhythmNT) {
            double s = extra[m];
            for (int f = 0; f < frames; ++f) s += R[f * ld + m] / len[f];
            extra[m] = s;
        }
    } else {
        for (int w = tid; w < frames * kRhythmRed; w += kRhythmNT) {
            const int f = w / kRhythmRed, l = w - f * kRhythmRed;
            double bv = 0.0;
            int bi = -1;
            for (int m = l; m < W; m += kRhythmRed) {
                const double s = rhythm_score(R[f * ld + m] / len[f], a.logprior[m]);
                if (rhythm_better(s, m, bv, bi)) { bv = s; bi = m; }
            }
            red[w] = bv;
            redi[w] = bi;
        }
        __syncthreads();
        for (int f = tid; f < frames; f += kRhythmNT) {
            double bv = 0.0;
            int bi = -1;
            for (int l = 0; l < kRhythmRed; ++l) {
                const int i = redi[f * kRhythmRed + l];
                if (i >= 0 && rhythm_better(red[f * kRhythmRed + l], i, bv, bi)) { bv = red[f * kRhythmRed + l]; bi = i; }
            }
            a.out[clip * a.n_frames + t0 + f] = a.bpms[bi];
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void rhythm_prologue(const Args& a, char* lds, const Lds& L) {
    if (a.mode == kSum) {
        double* extra = reinterpret_cast<double*>(lds + L.extra);
        for (int m = (int)threadIdx.x; m < a.W; m += kRhythmNT) extra[m] = 0.0;
    }
}

// after the group's chunks: the staged tile, lag row by lag row (lanes along frames), or the group's sums
__device__ __forceinline__ void rhythm_finish_group(const Args& a, char* lds, const Lds& L, long long clip, int group, int gframes) {
    const double* extra = reinterpret_cast<const double*>(lds + L.extra);
    const long long t0 = (long long)group * kRhythmGroup;
    if (a.mode == kWrite && a.tile) {
        for (int w = (int)threadIdx.x; w < a.W * kRhythmGroup; w += kRhythmNT) {
            const int m = w / kRhythmGroup, f = w - m * kRhythmGroup;
            if (f < gframes) a.out[(clip * a.W + m) * a.n_frames + t0 + f] = extra[w];
        }
    } else if (a.mode == kSum) {
        double* p = a.partial + (clip * a.groups + group) * (long long)a.W;
        for (int m = (int)threadIdx.x; m < a.W; m += kRhythmNT) p[m] = extra[m];
    }
}

// the transform of length N (in lra_mixed_sizes.h's size list)
template <int N> __device__ __forceinline__ void tempogram_fft_body(const Args& a) {
    constexpr int M = N / 2, FC = chunk_frames<N>(), HP = M / 2 + 1;
    LRA_RHYTHM_DYN_LDS(lds);
    const Lds L = lds_layout(N, a.W, a.mode, a.tile != 0);
    cpx<double>* buf0 = reinterpret_cast<cpx<double>*>(lds);
    cpx<double>* buf1 = buf0 + FC * M;
    cpx<double>* twm = buf1 + FC * M;
    const long long clip = blockIdx.x / (unsigned)a.groups;
    const int group = (int)(blockIdx.x % (unsigned)a.groups);
    const long long g0 = (long long)group * kRhythmGroup;
    const int gframes = (int)(a.n_frames - g0 < kRhythmGroup ? a.n_frames - g0 : kRhythmGroup);
    const int tid = (int)threadIdx.x;
    for (int t = tid; t < M; t += kRhythmNT) twm[t] = a.tw_m[t];
    rhythm_prologue(a, lds, L);
    for (int c0 = 0; c0 < gframes; c0 += FC) {
        const int frames = gframes - c0 < FC ? gframes - c0 : FC;
        // (1) window-multiplied frames packed as pairs z[j] = x[2j] + i x[2j + 1], zero beyond W
        for (int w = tid; w < frames * M; w += kRhythmNT) {
            const int f = w / M, j = w - f * M, n0 = 2 * j;
            const long long q = g0 + c0 + f + n0;  // padded position of the pair's first sample
            const double x0 = n0 < a.W ? rhythm_sample(a, clip, q) * a.win[n0] : 0.0;
            const double x1 = n0 + 1 < a.W ? rhythm_sample(a, clip, q + 1) * a.win[n0 + 1] : 0.0;
            buf0[w] = mkc<double>(x0, x1);
        }
        __syncthreads();
        // (2) forward M-point transform
        cpx<double>* src = buf0;
        cpx<double>* dst = buf1;
        mixed::Passes<double, N, 0, FC>::run(src, dst, twm, frames);
        // (3) per bin pair (k, M - k): Hermitian split -> X[k], X[M - k] -> |X|^2 -> the un-split of the inverse (lra_mixed.h unsplit_stage with a
        //     real spectrum): conj Z'[k] and conj Z'[M - k] into the other buffer
        for (int w = tid; w < frames * HP; w += kRhythmNT) {
            const int f = w / HP, k = w - f * HP;
            const cpx<double> wn = a.tw_n[k];
            const cpx<double> zk = src[f * M + k], zr = src[f * M + (k == 0 ? 0 : M - k)];
            const cpx<double> e = mkc<double>(0.5 * (zk.x + zr.x), 0.5 * (zk.y - zr.y)), o = mkc<double>(0.5 * (zk.x - zr.x), 0.5 * (zk.y + zr.y));
            const cpx<double> pw = mixed::mul(o, wn);
            cpx<double> xk = mkc<double>(e.x + pw.y, e.y - pw.x), xm = mkc<double>(e.x - pw.y, -e.y - pw.x);
            if (k == 0) { xk.y = 0.0; xm.y = 0.0; }
            const double p0 = fma_t(xk.y, xk.y, xk.x * xk.x), p1 = fma_t(xm.y, xm.y, xm.x * xm.x);
            const double ee = p0 + p1, d = p0 - p1;
            const cpx<double> od = mkc<double>(d * wn.x, -(d * wn.y));  // d conj(W_N^k)
            dst[f * M + k] = mkc<double>(ee - od.y, -od.x);
            if (k > 0 && 2 * k != M) dst[f * M + M - k] = mkc<double>(ee + od.y, -od.x);
        }
        __syncthreads();
        // (4) the inverse: forward passes on conj Z' give conj(M r) as pairs (r[2j], r[2j + 1]) = (Y.x, -Y.y) / N
        {
            cpx<double>* t = src;
            src = dst;
            dst = t;
        }
        mixed::Passes<double, N, 0, FC>::run(src, dst, twm, frames);
        double* R = reinterpret_cast<double*>(dst);  // rows of pitch N doubles in the free buffer
        for (int w = tid; w < frames * M; w += kRhythmNT) {
            const int f = w / M, j = w - f * M;
            if (2 * j < a.W) {
                const cpx<double> y = src[w];
                R[f * N + 2 * j] = y.x / (double)N;
                if (2 * j + 1 < a.W) R[f * N + 2 * j + 1] = -y.y / (double)N;
            }
        }
        __syncthreads();
        rhythm_epilogue(a, lds, L, R, N, frames, clip, group, c0);
    }
    rhythm_finish_group(a, lds, L, clip, group, gframes);
}

// any W (the host takes it where 2 W - 1 exceeds the transform sizes): r[m] = sum_j x[j] x[j + m], one frame at a time, same epilogues
__device__ __forceinline__ void tempogram_direct_body(const Args& a) {
    LRA_RHYTHM_DYN_LDS(lds);
    const Lds L = lds_layout(0, a.W, a.mode, a.tile != 0);
    double* x = reinterpret_cast<double*>(lds);
    double* R = x + a.W;
    const long long clip = blockIdx.x / (unsigned)a.groups;
    const int group = (int)(blockIdx.x % (unsigned)a.groups);
    const long long g0 = (long long)group * kRhythmGroup;
    const int gframes = (int)(a.n_frames - g0 < kRhythmGroup ? a.n_frames - g0 : kRhythmGroup);
    rhythm_prologue(a, lds, L);
    for (int c0 = 0; c0 < gframes; ++c0) {
        for (int n = (int)threadIdx.x; n < a.W; n += kRhythmNT) x[n] = rhythm_sample(a, clip, g0 + c0 + n) * a.win[n];
        __syncthreads();
        for (int m = (int)threadIdx.x; m < a.W; m += kRhythmNT) {
            double s = 0.0;
            for (int j = 0; j + m < a.W; ++j) s = fma_t(x[j], x[j + m], s);
            R[m] = s;
        }
        __syncthreads();
        rhythm_epilogue(a, lds, L, R, a.W, 1, clip, group, c0);
    }
    rhythm_finish_group(a, lds, L, clip, group, gframes);
}

// grid = batch * groups workgroups of kRhythmNT threads; dynamic LDS = lds_layout(N, W, mode, tile).total.  N = 0: the direct sum.
template <int N> __global__ __launch_bounds__(kRhythmNT) void tempogram_kernel(Args a) {
    if constexpr (N == 0) tempogram_direct_body(a);
    else tempogram_fft_body<N>(a);
}

// tempo with aggregate=np.mean: the groups' sums added in group order, / n_frames, log1p(1e6 mean) + logprior, np.argmax -> bpms.  grid = batch, block 256.
struct FinishArgs {
    const double* partial;   // [batch][groups][W]
    const double* logprior;  // [W]
    const double* bpms;      // [W]
    double* out;             // [batch]
    long long n_frames;
    int groups, W;
};
template <class T> __global__ __launch_bounds__(256) void tempo_mean_finish_kernel(FinishArgs a) {
    __shared__ T sv[256];
    __shared__ int si[256];
    const long long clip = blockIdx.x;
    const int tid = (int)threadIdx.x;
    double bv = 0.0;
    int bi = -1;
    for (int m = tid; m < a.W; m += 256) {
        T s = 0.0;
        for (int g = 0; g < a.groups; ++g) s += a.partial[(clip * a.groups + g) * (long long)a.W + m];
        const double sc = rhythm_score(s / (double)a.n_frames, a.logprior[m]);
        if (rhythm_better(sc, m, bv, bi)) { bv = sc; bi = m; }
    }
    sv[tid] = bv;
    si[tid] = bi;
    __syncthreads();
    if (tid == 0) {
        bv = 0.0;
        bi = -1;
        for (int l = 0; l < 256; ++l)
            if (si[l] >= 0 && rhythm_better(sv[l], si[l], bv, bi)) { bv = sv[l]; bi = si[l]; }
        a.out[clip] = a.bpms[bi];
    }
}

}  // namespace rhythm
}  // namespace lra
