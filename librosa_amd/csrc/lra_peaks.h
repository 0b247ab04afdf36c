// lra_peaks.h -- peak picking and onset backtracking: librosa.util.peak_pick's three kernels (librosa/util/utils.py:1183-1281), the
// normalisation of librosa.onset.onset_detect (librosa/onset.py:164-176) and onset_backtrack's preceding minimum (:430-441).
// Self-contained so that tests/hostsim/peaksim.cpp can run the same kernel bodies on host threads (-DLRA_POSTSIM).
//
// Launches on [batch][n] rows (T = float or double):
//   peak_stats_kernel        per row: min, x - min, max of that, / (max + tiny), each one rounding in T as NumPy does them (normalize = 0: a
//                            copy), and the two facts onset_detect asks of the whole array: some entry non-zero, some entry non-finite.
//   peak_candidates_kernel   one thread per frame: x[i] == max(x[i - pre_max : i + post_max]) (np.max hands a NaN on; the dp methods use the
//                            reference's `not (x[i] < max)`), and x[i] >= mean(x[i - pre_avg : i + post_avg]) + delta with the mean and the
//                            comparison in float64, summed first frame to last: the order depends on the frame index alone, so a row alone
//                            gives the bits of that row in a batch.  The row goes through LDS in tiles of kTile frames with kHalo frames on
//                            either side; a window that reaches further is read from global memory by the same loop.
//   peak_greedy_kernel       one wave per row: the reference's loop is earliest-first selection over the candidate flags with `wait` dead
//                            frames after a pick.  Per 64 frames one ballot; the mask is walked by count-trailing-zeros (peak_walk), "next
//                            allowed frame" is carried from chunk to chunk, every lane stores its own byte.
//   peak_dp_kernel           one wave per row: the backward recurrence of :1244-1275 in float64, values[i] = max(values[i + 1],
//                            values[min(n, i + wait + 1)] + v) over the candidates with v = 1 (dp_count) or x[i] cast up (dp_value), the
//                            sums in the reference's order and `>` deciding.  Lanes stage 64 frames, lane 0 runs them; the last kRing values
//                            live in LDS, and when wait + 1 exceeds the ring every value is also written to global scratch and read from
//                            there.  pointers[i] is n + wait + 1 for a taken frame and i + 1 otherwise, so the forward walk along the
//                            pointers is peak_walk again, over the taken masks.
//   prev_minimum_kernel      one wave per row: out[i] = the largest j <= i with j == 0 or (1 <= j <= m - 2, e[j] <= e[j - 1], e[j] < e[j + 1]):
//                            a ballot of the flags, and every lane takes the highest set bit at or below itself, else the carry.
// Every loop is bounded by the row length or by 64.
#pragma once

#ifndef LRA_POSTSIM
#include <hip/hip_runtime.h>
#endif

// one rounding per operation, as NumPy's arithmetic (hipcc contracts a * b + c into fma by default)
#pragma clang fp contract(off)

namespace lra {
namespace peaks {

constexpr int kGreedy = 0, kDpCount = 1, kDpValue = 2;  // the LRA_PEAK_* values of include/librosa_amd.h
constexpr int kStatsNT = 256;
constexpr int kTile = 256;   // frames per workgroup of peak_candidates_kernel (= its threads)
constexpr int kHalo = 64;    // frames of the neighbouring tiles kept in LDS on either side
constexpr int kWave = 64;    // threads of the one-wave kernels
constexpr int kRing = 2048;  // dp values kept in LDS (a power of two)

struct Args {
    const void* x;  // [batch][n] T
    long long n;
    int normalize;
    int pre_max, post_max, pre_avg, post_avg, wait;  // each at most n (clamp_window): a longer window or dead time is the same as n
    double delta;
    int method;
    void* norm;                 // [batch][n] T: the normalised rows (a copy with normalize = 0); the candidates are taken from these
    unsigned char* cand;        // [batch][n] scratch: candidate flags
    double* values;             // [batch][n + 1] scratch (dp)
    unsigned long long* taken;  // [batch][ceil(n / 64)] scratch (dp): bit l of word c = frame 64 c + l is taken
    int* status;                // [2] zeroed by the caller: [0] = 1 some entry of norm is non-zero, [1] = 1 some entry is not finite
    unsigned char* out;         // [batch][n] 1 = peak
};

inline long long clamp_window(long long v, long long n) { return v < 0 ? 0 : (v > n ? n : v); }

template <class T> struct Tiny;
template <> struct Tiny<float> { static constexpr float value = 1.17549435e-38f; };
template <> struct Tiny<double> { static constexpr double value = 2.2250738585072014e-308; };

#ifdef LRA_POSTSIM
unsigned long long peaks_wave_ballot(int pred);
#else
__device__ __forceinline__ unsigned long long peaks_wave_ballot(int pred) { return __ballot(pred); }
#endif

// min or max over the workgroup of values without NaN, and "some value was NaN" (np.min / np.max then return NaN)
template <bool kMax> __device__ __forceinline__ double peaks_block_extreme(double v, int nan, double* red, int* redi, int tid) {
    red[tid] = v;
    redi[tid] = nan;
    __syncthreads();
    for (int h = kStatsNT / 2; h > 0; h >>= 1) {
        if (tid < h) {
            const double o = red[tid + h];
            if (kMax ? o > red[tid] : o < red[tid]) red[tid] = o;
            redi[tid] |= redi[tid + h];
        }
        __syncthreads();
    }
    const double r = redi[0] ? __builtin_nan("") : red[0];
    __syncthreads();
    return r;
}

// grid = batch, block = kStatsNT
template <class T> __global__ __launch_bounds__(kStatsNT) void peak_stats_kernel(Args a) {
    __shared__ double red[kStatsNT];
    __shared__ int redi[kStatsNT];
    const long long row = blockIdx.x, n = a.n;
    const int tid = (int)threadIdx.x;
    const T* x = reinterpret_cast<const T*>(a.x) + row * n;
    T* xn = reinterpret_cast<T*>(a.norm) + row * n;
    const double inf = __builtin_inf();
    T mn = (T)0, den = (T)1;
    if (a.normalize) {
        double m = inf;
        int nan = 0;
        for (long long i = tid; i < n; i += kStatsNT) {
            const double v = (double)x[i];
            if (v != v) nan = 1;
            else m = v < m ? v : m;
        }
        mn = (T)peaks_block_extreme<false>(m, nan, red, redi, tid);
        m = -inf;
        nan = 0;
        for (long long i = tid; i < n; i += kStatsNT) {
            const T d = x[i] - mn;
            if (d != d) nan = 1;
            else m = (double)d > m ? (double)d : m;
        }
        den = (T)peaks_block_extreme<true>(m, nan, red, redi, tid) + Tiny<T>::value;
    }
    int nz = 0, bad = 0;
    for (long long i = tid; i < n; i += kStatsNT) {
        T v = x[i];
        if (a.normalize) {
            v = v - mn;
            v = v / den;
        }
        xn[i] = v;
        nz |= v != (T)0;              // (NaN counts as non-zero, as ndarray.any does)
        bad |= !(v - v == (T)0);      // inf - inf and NaN - NaN are NaN
    }
    redi[tid] = nz | (bad << 1);
    __syncthreads();
    for (int h = kStatsNT / 2; h > 0; h >>= 1) {
        if (tid < h) redi[tid] |= redi[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        if (redi[0] & 1) a.status[0] = 1;
        if (redi[0] & 2) a.status[1] = 1;
    }
}

// frame i of a row whose frame g is src[g - off] (only frames of the two windows are read)
template <class T> __device__ __forceinline__ unsigned char peak_is_candidate(const T* src, long long off, long long i, const Args& a) {
    const long long n = a.n;
    const T xi = src[i - off];
    long long lo = i - a.pre_max > 0 ? i - a.pre_max : 0, hi = i + a.post_max < n ? i + a.post_max : n;
    T m = src[lo - off];
    bool nan = m != m;
    for (long long g = lo + 1; g < hi; ++g) {
        const T v = src[g - off];
        nan |= v != v;
        m = v > m ? v : m;
    }
    // without a NaN the window's maximum is at least x[i], so `not (x[i] < max)` is `x[i] == max`; with one, == fails and `not <` holds
    const bool is_max = nan ? a.method != kGreedy : xi == m;
    lo = i - a.pre_avg > 0 ? i - a.pre_avg : 0;
    hi = i + a.post_avg < n ? i + a.post_avg : n;
    double s = 0.0;
    for (long long g = lo; g < hi; ++g) s += (double)src[g - off];
    const double mean = s / (double)(hi - lo);
    return is_max && (double)xi >= mean + a.delta;
}

// grid = batch * ceil(n / kTile), block = kTile: one frame per thread
template <class T> __global__ __launch_bounds__(kTile) void peak_candidates_kernel(Args a) {
    __shared__ T tile[kTile + 2 * kHalo];
    const long long n = a.n, tiles = (n + kTile - 1) / kTile;
    const long long row = blockIdx.x / tiles;
    const long long t0 = ((long long)blockIdx.x - row * tiles) * kTile;
    const int tid = (int)threadIdx.x;
    const T* x = reinterpret_cast<const T*>(a.norm) + row * n;
    const bool fits = a.pre_max <= kHalo && a.pre_avg <= kHalo && a.post_max <= kHalo && a.post_avg <= kHalo;  // (the same for every thread)
    if (fits)
        for (int j = tid; j < kTile + 2 * kHalo; j += kTile) {
            const long long g = t0 - kHalo + j;
            tile[j] = g >= 0 && g < n ? x[g] : (T)0;
        }
    __syncthreads();
    const long long i = t0 + tid;
    if (i >= n) return;
    // (two calls, so that each reads its own address space: LDS with the tile's first frame as offset, or the row itself)
    a.cand[row * n + i] = fits ? peak_is_candidate(tile, t0 - kHalo, i, a) : peak_is_candidate(x, 0, i, a);
}

// The picks among the flagged frames base .. base + 63 (bit l of m = frame base + l): the earliest frame at or after `next`, then the
// earliest at least wait + 1 later, and so on; `next` moves on with them.  The same for every lane of a wave; at most 64 rounds.
__device__ __forceinline__ unsigned long long peak_walk(unsigned long long m, long long base, long long& next, long long wait) {
    const long long k0 = next - base;
    if (k0 >= 64) return 0;
    if (k0 > 0) m &= ~0ull << k0;
    unsigned long long picks = 0;
    while (m) {
        const int p = __builtin_ctzll(m);
        picks |= 1ull << p;
        const long long k = p + wait + 1;
        next = base + k;
        m = k >= 64 ? 0 : m & (~0ull << k);
    }
    return picks;
}

// grid = batch, block = kWave (a template like the others, though it reads no T: the header serves more than one translation unit)
template <class T> __global__ __launch_bounds__(kWave) void peak_greedy_kernel(Args a) {
    const long long row = blockIdx.x, n = a.n;
    const int lane = (int)threadIdx.x;
    const unsigned char* cand = a.cand + row * n;
    unsigned char* out = a.out + row * n;
    long long next = 0;
    for (long long base = 0; base < n; base += kWave) {
        const long long i = base + lane;
        const unsigned long long m = peaks_wave_ballot(i < n && cand[i]);
        const unsigned long long picks = peak_walk(m, base, next, a.wait);
        if (i < n) out[i] = (unsigned char)((picks >> lane) & 1);
    }
}

// grid = batch, block = kWave
template <class T> __global__ __launch_bounds__(kWave) void peak_dp_kernel(Args a) {
    __shared__ double ring[kRing];
    __shared__ double sv[kWave];
    const long long row = blockIdx.x, n = a.n, chunks = (n + kWave - 1) / kWave;
    const int lane = (int)threadIdx.x;
    const T* x = reinterpret_cast<const T*>(a.norm) + row * n;
    const unsigned char* cand = a.cand + row * n;
    double* values = a.values + row * (n + 1);
    unsigned long long* taken = a.taken + row * chunks;
    unsigned char* out = a.out + row * n;
    const long long wait = a.wait;
    const bool near = wait + 1 <= kRing;  // every value read is still in the ring (read before the frame's own slot is overwritten)
    if (lane == 0) {
        ring[n & (kRing - 1)] = 0.0;
        if (!near) values[n] = 0.0;
    }
    double vnext = 0.0;  // values[i + 1] (lane 0)
    for (long long base = (chunks - 1) * kWave; base >= 0; base -= kWave) {
        const long long i = base + lane;
        int c = 0;
        if (i < n) {
            c = cand[i];
            sv[lane] = a.method == kDpCount ? 1.0 : (double)x[i];
        }
        const unsigned long long m = peaks_wave_ballot(c);
        __syncthreads();
        if (lane == 0) {
            unsigned long long tk = 0;
            const int top = n - base < kWave ? (int)(n - base) - 1 : kWave - 1;
            for (int l = top; l >= 0; --l) {
                const long long f = base + l;
                double val = vnext;
                if ((m >> l) & 1) {
                    const long long j = f + wait + 1 < n ? f + wait + 1 : n;
                    const double s = (near ? ring[j & (kRing - 1)] : values[j]) + sv[l];
                    if (s > vnext) {
                        val = s;
                        tk |= 1ull << l;
                    }
                }
                ring[f & (kRing - 1)] = val;
                if (!near) values[f] = val;
                vnext = val;
            }
            taken[base / kWave] = tk;
        }
        __syncthreads();
    }
    long long next = 0;
    for (long long base = 0; base < n; base += kWave) {
        const long long i = base + lane;
        const unsigned long long picks = peak_walk(taken[base / kWave], base, next, wait);
        if (i < n) out[i] = (unsigned char)((picks >> lane) & 1);
    }
}

struct MinArgs {
    const void* energy;  // [batch][m] T
    long long m;
    int* out;            // [batch][m]
};

// grid = batch, block = kWave
template <class T> __global__ __launch_bounds__(kWave) void prev_minimum_kernel(MinArgs a) {
    const long long row = blockIdx.x, m = a.m;
    const int lane = (int)threadIdx.x;
    const T* e = reinterpret_cast<const T*>(a.energy) + row * m;
    int* out = a.out + row * m;
    long long carry = 0;
    for (long long base = 0; base < m; base += kWave) {
        const long long i = base + lane;
        int f = 0;
        if (i == 0) f = 1;
        else if (i <= m - 2) f = e[i] <= e[i - 1] && e[i] < e[i + 1];
        const unsigned long long mask = peaks_wave_ballot(f);
        const unsigned long long below = mask & (lane == 63 ? ~0ull : (2ull << lane) - 1);
        if (i < m) out[i] = (int)(below ? base + 63 - __builtin_clzll(below) : carry);
        if (mask) carry = base + 63 - __builtin_clzll(mask);
    }
}

}  // namespace peaks
}  // namespace lra

#pragma clang fp contract(fast)
