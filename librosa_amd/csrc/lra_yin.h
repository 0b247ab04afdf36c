// lra_yin.h -- librosa.yin (librosa/core/pitch.py:369-628) and the front half it shares with pyin: the cumulative mean normalised difference
// function of every frame and the parabolic shifts, in one launch that reads the samples once.
// Self-contained so that tests/hostsim/yinsim.cpp can run the same kernel bodies on host threads (-DLRA_POSTSIM).
//
//   frame t = padded[t * hop : t * hop + W]                              (centre padding folded into the load index; float64 from here on)
//   d(k)    = 2 (acf(0) - acf(k)) - E(k - 1),  k = 1 .. P                (P = max_period; E = cumsum(y^2) with E(0) read as 0: the reference
//                                                                         clears yin_frames[0] before it reads the energies back)
//   c(i)    = d(k) / (sum(d(1 .. k)) / k + tiny),  k = p0 + i            (p0 = min_period, i = 0 .. P - p0)
//   trough  : c(i) < c(i - 1) and c(i) <= c(i + 1); c(0) < c(1) at the first lag; c(last) < c(last - 1) at the last (util.localmin)
//   index   = the first trough with c < trough_threshold, else np.argmin(c)
//   shift   = -b / a of the parabola through c(i - 1 .. i + 1), 0 where |b| >= |a| and at both ends
//   f0      = sr / (p0 + index + shift)
//
// A workgroup of 256 threads owns kYinGroup consecutive frames of one clip.
//   yin_kernel<N>   acf(0 .. P) through the real transform of length N >= W + P (no wrap-around up to lag P) on the Stockham passes of
//                   lra::mixed, chunk_frames_of(N) frames at a time: the frame packed as N / 2 complex points, the forward passes, one stage
//                   for the Hermitian split, |X|^2 and the un-split of the inverse, the forward passes again on the conjugate (as
//                   lra_rhythm.h).  The running energies are summed from the packed frame before the first pass overwrites it.  The next
//                   chunk's samples are loaded into registers before the passes of this one.
//   yin_kernel<0>   any W: d(k) = sum_{j < W - k} (y_j - y_{j + k})^2 + sum_{j >= W - k} y_j^2 (+ y_0^2 at k = 1), the same number without
//                   the cancellation, one frame at a time from the cached samples.  Its two rows of lags take 16 max_period bytes of LDS:
//                   max_period <= 10239 (the host refuses longer ones).
// Both continue with the prefix sums of d (a wave per frame, a run of lags per lane, the runs' totals scanned by shuffles) and the CMND in LDS.
// Two epilogues, chosen at run time:
//   F0      one float64 per frame; nothing dense is written.
//   FRAMES  c and the shifts of every lag as [clip][lag][frame] in the input's type (what pyin reads).  A chunk's frames are adjacent in a lag row;
//           from N = 1600 on and in the direct kernel a chunk is one frame, and every lane stores one element n_frames apart.
// The order of every addition depends on W, P and N alone, so a clip gives the same bits alone and inside a batch.
#pragma once

#ifndef LRA_POSTSIM
#include <hip/hip_runtime.h>
#endif

#include "lra_mixed.h"
#include "lra_mixed_sizes.h"

#ifdef LRA_POSTSIM
#define LRA_YIN_DYN_LDS(ptr) char* ptr = reinterpret_cast<char*>(g_postsim_dyn_lds)
#else
#define LRA_YIN_DYN_LDS(ptr) extern __shared__ __align__(16) char lra_yin_lds[]; char* ptr = lra_yin_lds
#endif

namespace lra {
namespace yin {

using mixed::cpx;
using mixed::fma_t;
using mixed::mkc;

constexpr int kF0 = 0, kFrames = 1;  // the LRA_YIN_* values of include/librosa_amd.h
constexpr int kYinNT = mixed::NT;    // threads per workgroup (the passes deal their work items over this many)
constexpr int kYinGroup = 16;        // frames per workgroup (a FRAMES lag row gets a run of chunk_frames_of(N) of them at a time: 16 only at N = 160)
constexpr int kYinRed = 64;          // lanes per frame in the prefix sums and the selection
constexpr int kYinLdsMax = 160 * 1024;
constexpr int kYinChunkLds = 48 * 1024;  // what the transform's ping-pong buffers of a chunk may take

// frames transformed at a time: two ping-pong buffers of N / 2 complex doubles per frame within kYinChunkLds (a power of two dividing the group)
constexpr int chunk_frames_of(int N) {
    int fc = kYinGroup;
    while (fc > 1 && fc * 2 * (N / 2) * 16 > kYinChunkLds) fc /= 2;
    return fc;
}
template <int N> constexpr int chunk_frames() { return chunk_frames_of(N); }

// LDS layout (bytes, host and device): [FFT buffers | direct: the d row] [P sums per frame: energies, then sums of d]
struct Lds {
    int sums, total;
};
constexpr Lds lds_layout(int N, int P) {
    Lds l{};
    const int fc = N > 0 ? chunk_frames_of(N) : 1;
    l.sums = N > 0 ? 2 * fc * (N / 2) * 16 : (P + 1) * 8;
    l.total = l.sums + fc * P * 8;
    return l;
}

struct Args {
    const void* y;           // [batch][n] float32 or float64 (y_f64)
    int y_f64;
    long long n;             // samples per clip
    long long n_frames;      // 1 + (n + 2 pad - W) / hop
    int W, hop, pad;         // pad = W / 2 (centre) or 0
    int pad_mode;            // 0 constant, 1 reflect, 2 edge, 3 symmetric (np.pad)
    int N;                   // transform length (0: direct kernel)
    int min_period, max_period;
    double threshold, sr, tiny;
    const cpx<double>* tw_m; // [N / 2]     W_M^t
    const cpx<double>* tw_n; // [N / 2 + 1] W_N^k
    int mode;
    double* f0;              // F0: [batch][n_frames]
    void* frames;            // FRAMES: [batch][max_period - min_period + 1][n_frames] in the input's type
    void* shifts;            // FRAMES: the same shape
    int groups;              // ceil(n_frames / kYinGroup)
};

// the smallest size of LRA_MIXED_SIZES that holds the linear autocorrelation of W samples up to lag P (W + P), or 0: the direct kernel
constexpr int transform_length(int W, int P) { return mixed::smallest_size_at_least(W + P); }

// Host: the geometry of one lra_yin_exec call, from its scalar parameters into a (the pointers and y_f64 stay the caller's).  Answers
// mixed::kGeometryTooShort (only W, hop and pad set: the padded clip does not hold one frame) or, everything set, mixed::kGeometryLds (max_period
// does not fit the LDS of a workgroup).  direct: the direct kernel whatever the size list offers -- the host simulator's switch.
inline int prepare(Args& a, long long n, int W, int hop, int center, int pad_mode, int min_period, int max_period, double threshold, double sr, int mode, bool direct = false) {
    a.W = W;
    a.hop = hop;
    a.pad = center ? W / 2 : 0;
    if (n + 2 * (long long)a.pad < W) return mixed::kGeometryTooShort;
    a.n = n;
    a.n_frames = 1 + (n + 2 * (long long)a.pad - W) / hop;
    a.pad_mode = pad_mode;
    a.N = direct ? 0 : transform_length(W, max_period);
    a.min_period = min_period;
    a.max_period = max_period;
    a.threshold = threshold;
    a.sr = sr;
    a.tiny = 2.2250738585072014e-308;  // util.tiny of the float64 cumulative mean (the division by the int64 lags promotes a float32 frame)
    a.mode = mode;
    a.groups = (int)((a.n_frames + kYinGroup - 1) / kYinGroup);
    return lds_layout(a.N, max_period).total > kYinLdsMax ? mixed::kGeometryLds : mixed::kGeometryOk;
}

// sample q of the padded clip (np.pad's modes as lra::mixed::fetch)
__device__ __forceinline__ double yin_sample(const Args& a, long long clip, long long q) {
    long long g = q - a.pad;
    const long long n = a.n;
    if (g < 0 || g >= n) {
        if (n <= 0 || a.pad_mode == 0) return 0.0;
        if (a.pad_mode == 2 || n == 1) g = g < 0 ? 0 : n - 1;
        else {
            const long long lo = a.pad_mode == 1 ? 0 : -1, hi = a.pad_mode == 1 ? 2 * (n - 1) : 2 * n - 1;
            while (g < 0 || g >= n) g = g < 0 ? lo - g : hi - g;
        }
    }
    const long long at = clip * n + g;
    return a.y_f64 ? reinterpret_cast<const double*>(a.y)[at] : (double)reinterpret_cast<const float*>(a.y)[at];
}

#ifdef LRA_POSTSIM
double yin_shfl_up(double v, int delta);   // the value of lane (lane - delta) of the same wave; the lane's own below delta
double yin_shfl_xor(double v, int offset); // the value of lane (lane ^ offset) of the same wave
int yin_shfl_xor(int v, int offset);
#else
__device__ __forceinline__ double yin_shfl_up(double v, int delta) { return __shfl_up(v, (unsigned)delta, 64); }
__device__ __forceinline__ double yin_shfl_xor(double v, int offset) { return __shfl_xor(v, offset, 64); }
__device__ __forceinline__ int yin_shfl_xor(int v, int offset) { return __shfl_xor(v, offset, 64); }
#endif

// np.argmin's order: the first NaN wins; otherwise the smaller value, the lower index on a tie; bi < 0: nothing taken yet
__device__ __forceinline__ bool yin_better(double v, int i, double bv, int bi) {
    if (bi < 0) return true;
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v < bv || (v == bv && i < bi);
}

// util.localmin with yin's first-lag rule, on the L values c[0 .. L - 1] (L >= 2)
__device__ __forceinline__ bool yin_trough(const double* c, int i, int L) {
    if (i == 0) return c[0] < c[1];
    if (i == L - 1) return c[i] < c[i - 1];
    return c[i] < c[i - 1] && c[i] <= c[i + 1];
}

// _parabolic_interpolation: 0 at both ends and where the vertex is more than a bin away
__device__ __forceinline__ double yin_shift(const double* c, int i, int L) {
    if (i <= 0 || i >= L - 1) return 0.0;
    const double pa = c[i + 1] + c[i - 1] - 2.0 * c[i];
    const double pb = (c[i + 1] - c[i - 1]) / 2.0;
    return __builtin_fabs(pb) >= __builtin_fabs(pa) ? 0.0 : -pb / pa;
}

// Inclusive prefix sums of src(f, 0 .. P - 1) into dst[f * P + j]: a wave per frame, every lane sums a run of lags, the runs' totals are
// scanned across the wave (six shuffle steps) and each lane adds what lies before its run.  Ends with a barrier.
template <class Src> __device__ __forceinline__ void yin_scan(Src src, double* dst, int frames, int P) {
    const int tid = (int)threadIdx.x, seg = (P + kYinRed - 1) / kYinRed;
    for (int w = tid; w < frames * kYinRed; w += kYinNT) {  // (w / kYinRed is the same for a whole wave: its lanes shuffle together)
        const int f = w / kYinRed, l = w - f * kYinRed;
        const int j0 = l * seg, j1 = j0 + seg < P ? j0 + seg : P;
        double s = 0.0;
        for (int j = j0; j < j1; ++j) {
            s += src(f, j);
            dst[f * P + j] = s;
        }
        for (int d = 1; d < kYinRed; d <<= 1) {
            const double o = yin_shfl_up(s, d);
            if (l >= d) s += o;
        }
        const double before = yin_shfl_up(s, 1);
        if (l > 0)
            for (int j = j0; j < j1; ++j) dst[f * P + j] = before + dst[f * P + j];
    }
    __syncthreads();
}

// From the difference functions of `frames` frames (d(k) at D[f * ld + k], k = 1 .. P) to the results of group frames c0 .. c0 + frames - 1.
// D is overwritten with the CMND.  Ends with a barrier: D and the sums may be overwritten afterwards.
__device__ __forceinline__ void yin_finish(const Args& a, char* lds, const Lds& L, double* D, int ld, int frames, long long clip, int group, int c0) {
    double* sums = reinterpret_cast<double*>(lds + L.sums);
    const int tid = (int)threadIdx.x, P = a.max_period, p0 = a.min_period, Lc = P - p0 + 1;
    const long long t0 = (long long)group * kYinGroup + c0;  // clip frame of D's first row
    yin_scan([=](int f, int j) { return D[f * ld + j + 1]; }, sums, frames, P);
    for (int w = tid; w < frames * Lc; w += kYinNT) {
        const int f = w / Lc, k = p0 + (w - f * Lc);
        D[f * ld + k] = D[f * ld + k] / (sums[f * P + k - 1] / (double)k + a.tiny);
    }
    __syncthreads();
    if (a.mode == kFrames) {
        for (int w = tid; w < frames * Lc; w += kYinNT) {
            const int i = w / frames, f = w - i * frames;  // the chunk's frames of a lag row side by side (one frame: a store per lane, n_frames apart)
            const double* c = D + f * ld + p0;
            const long long at = (clip * Lc + i) * a.n_frames + t0 + f;
            const double v = c[i], s = yin_shift(c, i, Lc);
            if (a.y_f64) {
                reinterpret_cast<double*>(a.frames)[at] = v;
                reinterpret_cast<double*>(a.shifts)[at] = s;
            } else {
                reinterpret_cast<float*>(a.frames)[at] = (float)v;
                reinterpret_cast<float*>(a.shifts)[at] = (float)s;
            }
        }
    } else {
        // a wave per frame: every lane keeps the first match and the minimum of its lags, a butterfly of shuffles joins them
        for (int w = tid; w < frames * kYinRed; w += kYinNT) {
            const int f = w / kYinRed, l = w - f * kYinRed;
            const double* c = D + f * ld + p0;
            double bv = 0.0;
            int bi = -1, fi = -1;
            for (int i = l; i < Lc; i += kYinRed) {
                const double v = c[i];
                if (fi < 0 && v < a.threshold && yin_trough(c, i, Lc)) fi = i;
                if (yin_better(v, i, bv, bi)) { bv = v; bi = i; }
            }
            for (int off = kYinRed / 2; off > 0; off >>= 1) {
                const double ov = yin_shfl_xor(bv, off);
                const int oi = yin_shfl_xor(bi, off), ofi = yin_shfl_xor(fi, off);
                if (oi >= 0 && yin_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
                if (ofi >= 0 && (fi < 0 || ofi < fi)) fi = ofi;
            }
            const int idx = fi >= 0 ? fi : bi;
            if (l == 0) a.f0[clip * a.n_frames + t0 + f] = a.sr / ((double)(p0 + idx) + yin_shift(c, idx, Lc));
        }
    }
    __syncthreads();
}

// the transform of length N (in lra_mixed_sizes.h's size list), N >= W + max_period
template <int N> __device__ __forceinline__ void yin_fft_body(const Args& a) {
    constexpr int M = N / 2, FC = chunk_frames<N>(), HP = M / 2 + 1, IT = (FC * M + kYinNT - 1) / kYinNT;
    LRA_YIN_DYN_LDS(lds);
    const Lds L = lds_layout(N, a.max_period);
    cpx<double>* buf0 = reinterpret_cast<cpx<double>*>(lds);
    cpx<double>* buf1 = buf0 + FC * M;
    const cpx<double>* twm = a.tw_m;  // read through the caches: the table in LDS would cost a workgroup per CU at the default frame
    double* sums = reinterpret_cast<double*>(lds + L.sums);
    const long long clip = blockIdx.x / (unsigned)a.groups;
    const int group = (int)(blockIdx.x % (unsigned)a.groups);
    const long long g0 = (long long)group * kYinGroup;
    const int gframes = (int)(a.n_frames - g0 < kYinGroup ? a.n_frames - g0 : kYinGroup);
    const int tid = (int)threadIdx.x, W = a.W, P = a.max_period;
    // a chunk's frames packed as pairs z[j] = x[2j] + i x[2j + 1], zero beyond W: work item w = tid + it * NT, held in registers
    cpx<double> pre[IT];
    auto load_chunk = [&](int c0, int frames) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int w = tid + it * kYinNT;
            pre[it] = mkc<double>(0.0, 0.0);
            if (w >= frames * M) continue;
            const int f = w / M, n0 = 2 * (w - f * M);
            const long long q = (g0 + c0 + f) * a.hop + n0;  // padded position of the pair's first sample
            const double x0 = n0 < W ? yin_sample(a, clip, q) : 0.0;
            const double x1 = n0 + 1 < W ? yin_sample(a, clip, q + 1) : 0.0;
            pre[it] = mkc<double>(x0, x1);
        }
    };
    load_chunk(0, gframes < FC ? gframes : FC);
    for (int c0 = 0; c0 < gframes; c0 += FC) {
        const int frames = gframes - c0 < FC ? gframes - c0 : FC;
        cpx<double>* src = buf0;
        cpx<double>* dst = buf1;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int w = tid + it * kYinNT;
            if (w < frames * M) src[w] = pre[it];
        }
        __syncthreads();
        // the next chunk's samples: issued now, stored at the top of the next trip
        if (c0 + FC < gframes) load_chunk(c0 + FC, gframes - c0 - FC < FC ? gframes - c0 - FC : FC);
        // (1) running energies E(j) = sum_{i <= j} y_i^2, j < P, while the packed frames are still there
        yin_scan([=](int f, int j) { const cpx<double> z = src[f * M + (j >> 1)]; const double v = (j & 1) ? z.y : z.x; return v * v; }, sums, frames, P);
        // (2) forward M-point transform
        mixed::Passes<double, N, 0, FC>::run(src, dst, twm, frames);
        // (3) per bin pair (k, M - k): Hermitian split -> X[k], X[M - k] -> |X|^2 -> the un-split of the inverse with a real spectrum
        for (int w = tid; w < frames * HP; w += kYinNT) {
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
        // (5) d(k) = 2 (r(0) - r(k)) - E(k - 1) into rows of pitch N doubles in the free buffer; E(0) reads as 0
        double* D = reinterpret_cast<double*>(dst);
        for (int w = tid; w < frames * P; w += kYinNT) {
            const int f = w / P, k = 1 + (w - f * P);
            const cpx<double> y0 = src[f * M], yk = src[f * M + (k >> 1)];
            const double r0 = y0.x / (double)N, rk = ((k & 1) ? -yk.y : yk.x) / (double)N;
            D[f * N + k] = 2.0 * (r0 - rk) - (k > 1 ? sums[f * P + k - 1] : 0.0);
        }
        __syncthreads();
        yin_finish(a, lds, L, D, N, frames, clip, group, c0);
    }
}

// any W: the cancellation-free form of d, one frame at a time, same finish
__device__ __forceinline__ void yin_direct_body(const Args& a) {
    LRA_YIN_DYN_LDS(lds);
    const Lds L = lds_layout(0, a.max_period);
    double* D = reinterpret_cast<double*>(lds);
    const long long clip = blockIdx.x / (unsigned)a.groups;
    const int group = (int)(blockIdx.x % (unsigned)a.groups);
    const long long g0 = (long long)group * kYinGroup;
    const int gframes = (int)(a.n_frames - g0 < kYinGroup ? a.n_frames - g0 : kYinGroup);
    const int W = a.W, P = a.max_period;
    for (int c0 = 0; c0 < gframes; ++c0) {
        const long long q0 = (g0 + c0) * a.hop;
        for (int k = 1 + (int)threadIdx.x; k <= P; k += kYinNT) {
            // thousands of terms in a row: a compensated sum (two-sum of the running total, the square's own rounding by fma), so that a long
            // frame stays as close to the exact value as the transform route does
            double d = 0.0, comp = 0.0;
            auto add_square = [&](double t) {
                const double p = fma_t(t, t, 0.0), pe = fma_t(t, t, -p);  // (spelled as fma: the product must not be contracted into the sum below)
                const double s2 = d + p, bb = s2 - d;
                comp += ((d - (s2 - bb)) + (p - bb)) + pe;
                d = s2;
            };
            for (int j = 0; j + k < W; ++j) add_square(yin_sample(a, clip, q0 + j) - yin_sample(a, clip, q0 + j + k));
            for (int j = W - k; j < W; ++j) add_square(yin_sample(a, clip, q0 + j));
            if (k == 1) add_square(yin_sample(a, clip, q0));
            d += comp;
            D[k] = d;
        }
        __syncthreads();
        yin_finish(a, lds, L, D, P + 1, 1, clip, group, c0);
    }
}

// grid = batch * groups workgroups of kYinNT threads; dynamic LDS = lds_layout(N, max_period).total.  N = 0: the direct sum.
template <int N> __global__ __launch_bounds__(kYinNT) void yin_kernel(Args a) {
    if constexpr (N == 0) yin_direct_body(a);
    else yin_fft_body<N>(a);
}

}  // namespace yin
}  // namespace lra
