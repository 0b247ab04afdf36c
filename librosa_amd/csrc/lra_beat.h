// lra_beat.h -- the dynamic-programming beat tracker: librosa.beat.beat_track's __beat_tracker (librosa/beat.py:510-741).
// Self-contained so that tests/hostsim/beatsim.cpp can run the same kernel bodies on host threads (-DLRA_POSTSIM).
//
// Three launches on [batch][n] onset envelopes (T = float or double):
//   beat_prepare_kernel      per row: the sample standard deviation (ddof=1), x / (std + tiny) in T (:567-570), frames_per_beat =
//                            round(frame_rate * 60 / bpm) in float64, half-even (:546), per row or per frame; "some entry is non-zero" (:280).
//   beat_local_score_kernel  one thread per frame: the same-mode convolution with exp(-0.5 (k 32 / fpb)^2), k = -fpb .. fpb (:576-608).  The
//                            reference adds every term to the stored T value, in increasing k; so does this loop (one rounding to T per term).
//   beat_track_kernel        one wave per row: the recurrence (:619-660) frame after frame, then the tail (:697-729), the walk along the
//                            back-links (:736-741) and the trim (:667-694).
// The recurrence is float64 whatever T is (the reference's float32 signature cannot take the float64 frames_per_beat, so the float64 one runs
// and casts the local score up); tightness is rounded to float32 first, as its signature says.  Candidates of frame i: loc = i - round(fpb / 2)
// (half-even) down to i - 2 fpb, stopping at 0; the best score wins, the largest loc on a tie.  With one tempo per row the penalty
// tightness (log(i - loc) - log(fpb))^2 depends on the distance alone: it is tabulated once in LDS, lanes deal the distances among themselves,
// and a frame costs one LDS read of each table, one subtraction and a cross-lane maximum.  The last kBeatRing values of the cumulative score
// live in LDS as a ring and every value is written through to global scratch, so the row length is not limited by LDS; a window wider than the
// ring (or a tempo per frame) takes the general loop: log on the fly, values beyond the ring from global memory.
// Every loop is bounded by the row length: the reference's back-track and trim loops are `while` loops over data; here a back-link that does
// not point backwards ends the walk, and the trim is two index reductions.
// Rows the reference cannot handle are defined here and get NO beats: n < 2 (IndexError in localmax), an all-zero row beside live rows (its
// trim loop walks off the array), and frames_per_beat < 2 or > kBeatMaxFpb (the candidate range then starts at the frame itself, whose score
// is not computed yet, or overflows).
#pragma once

#ifndef LRA_POSTSIM
#include <hip/hip_runtime.h>
#endif

// one rounding per operation, as NumPy's scalar arithmetic (hipcc contracts a * b + c into fma by default)
#pragma clang fp contract(off)

namespace lra {
namespace beat {

constexpr int kPerRow = 0, kPerFrame = 1;  // the LRA_BEAT_BPM_* values of include/librosa_amd.h
constexpr int kBeatWave = 64;              // threads of beat_track_kernel: one wave
constexpr int kBeatRing = 2048;            // cumulative scores kept in LDS (a power of two); also the penalty table's size
constexpr int kBeatPrepNT = 256;
constexpr double kBeatMaxFpb = 536870912.0;  // 2^29: 2 fpb fits an int

struct Args {
    const void* env;     // [batch][n] T
    long long n;
    const double* bpm;   // [batch] (kPerRow) or [batch][n] (kPerFrame)
    int bpm_mode;
    double frame_rate;   // sr / hop_length
    float tightness;
    int trim;
    void* norm;          // [batch][n] T   scratch: the normalised envelope
    void* local;         // [batch][n] T   scratch: the local score
    double* fpb;         // [batch] or [batch][n] scratch: frames per beat
    double* cum;         // [batch][n] scratch: the cumulative score
    int* backlink;       // [batch][n] scratch
    int* order;          // [batch][n] scratch: local-maximum flags, then the beats in the order the walk visits them
    int* dead;           // [batch] scratch: 1 = a row that gets no beats
    int* any;            // set to 1 when some entry of env is non-zero
    unsigned char* out;  // [batch][n] 1 = beat
};

template <class T> struct Tiny;
template <> struct Tiny<float> { static constexpr float value = 1.17549435e-38f; };
template <> struct Tiny<double> { static constexpr double value = 2.2250738585072014e-308; };

// ---- cross-lane helpers of the one-wave kernel (the simulator supplies its own) ----------------------------------------------------------
#ifdef LRA_POSTSIM
double beat_wave_max(double v);
long long beat_wave_max_ll(long long v);
long long beat_wave_sum_ll(long long v);
unsigned long long beat_wave_ballot(int pred);
int beat_wave_read(int v, int lane);
#else
__device__ __forceinline__ double beat_wave_max(double v) {
    for (int m = 32; m > 0; m >>= 1) {
        const double o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ long long beat_wave_max_ll(long long v) {
    for (int m = 32; m > 0; m >>= 1) {
        const long long o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ long long beat_wave_sum_ll(long long v) {
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ unsigned long long beat_wave_ballot(int pred) { return __ballot(pred); }
__device__ __forceinline__ int beat_wave_read(int v, int lane) { return __shfl(v, lane); }
#endif

// an order-preserving integer key of a double (for the median's bitwise selection) and back
__device__ __forceinline__ unsigned long long beat_key(double v) {
    unsigned long long b;
    __builtin_memcpy(&b, &v, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double beat_unkey(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    __builtin_memcpy(&v, &b, 8);
    return v;
}

__device__ __forceinline__ bool beat_fpb_ok(double f) { return f >= 2.0 && f <= kBeatMaxFpb; }

// grid = batch, block = kBeatPrepNT.  Sums in float64 in an order that depends on the frame index alone (a row alone = the row in a batch).
template <class T> __global__ __launch_bounds__(kBeatPrepNT) void beat_prepare_kernel(Args a) {
    __shared__ double red[kBeatPrepNT];
    __shared__ int redi[kBeatPrepNT];
    const long long row = blockIdx.x, n = a.n;
    const int tid = (int)threadIdx.x;
    const T* x = reinterpret_cast<const T*>(a.env) + row * n;
    T* xn = reinterpret_cast<T*>(a.norm) + row * n;
    double s = 0.0;
    int nz = 0;
    for (long long i = tid; i < n; i += kBeatPrepNT) {
        const T v = x[i];
        s += (double)v;
        nz |= v != (T)0;  // (NaN counts as non-zero, as ndarray.any does)
    }
    red[tid] = s;
    redi[tid] = nz;
    __syncthreads();
    for (int h = kBeatPrepNT / 2; h > 0; h >>= 1) {
        if (tid < h) {
            red[tid] += red[tid + h];
            redi[tid] |= redi[tid + h];
        }
        __syncthreads();
    }
    const double mean = red[0] / (double)n;
    const int row_any = redi[0];
    __syncthreads();
    double q = 0.0;
    for (long long i = tid; i < n; i += kBeatPrepNT) {
        const double d = (double)x[i] - mean;
        q += d * d;
    }
    red[tid] = q;
    __syncthreads();
    for (int h = kBeatPrepNT / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    const T sd = (T)sqrt(red[0] / (double)(n - 1));  // ddof = 1 (n = 1: NaN, and the row is dead)
    const T den = sd + Tiny<T>::value;
    for (long long i = tid; i < n; i += kBeatPrepNT) xn[i] = x[i] / den;
    int bad = 0;
    if (a.bpm_mode == kPerFrame) {
        for (long long i = tid; i < n; i += kBeatPrepNT) {
            const double f = rint(a.frame_rate * 60.0 / a.bpm[row * n + i]);
            a.fpb[row * n + i] = f;
            bad |= !beat_fpb_ok(f);
        }
    } else if (tid == 0) {
        const double f = rint(a.frame_rate * 60.0 / a.bpm[row]);
        a.fpb[row] = f;
        bad = !beat_fpb_ok(f);
    }
    __syncthreads();
    redi[tid] = bad;
    __syncthreads();
    for (int h = kBeatPrepNT / 2; h > 0; h >>= 1) {
        if (tid < h) redi[tid] |= redi[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        a.dead[row] = redi[0] || n < 2 || !row_any;
        if (row_any) *a.any = 1;
    }
}

// grid = batch * ceil(n / 256), block = 256: one output frame per thread
template <class T> __global__ __launch_bounds__(256) void beat_local_score_kernel(Args a) {
    const long long n = a.n, blocks = (n + 255) / 256;
    const long long row = blockIdx.x / blocks;
    const long long i = ((long long)blockIdx.x - row * blocks) * 256 + threadIdx.x;
    if (i >= n) return;
    T* ls = reinterpret_cast<T*>(a.local) + row * n;
    if (a.dead[row]) {
        ls[i] = (T)0;
        return;
    }
    const T* xn = reinterpret_cast<const T*>(a.norm) + row * n;
    const double f = a.bpm_mode == kPerFrame ? a.fpb[row * n + i] : a.fpb[row];
    const long long F = (long long)f, K = 2 * F + 1;
    // range(max(0, i + K // 2 - N + 1), min(i + K // 2, K)): at most n terms
    const long long k0 = i + F - n + 1 > 0 ? i + F - n + 1 : 0, k1 = i + F < K ? i + F : K;
    T acc = (T)0;
    for (long long k = k0; k < k1; ++k) {
        const double t = ((double)(k - F) * 32.0) / f;
        const double w = exp(-0.5 * (t * t));
        acc = (T)((double)acc + w * (double)xn[i + F - k]);
    }
    ls[i] = acc;
}

__device__ __forceinline__ int beat_is_localmax(const double* c, long long i, long long n) {
    if (i == 0) return 0;
    if (i == n - 1) return c[i] > c[i - 1];
    return c[i] > c[i - 1] && c[i] >= c[i + 1];
}

// the k-th smallest (0-based) cumulative score among the flagged frames: bit by bit from the top of the order-preserving key
__device__ __forceinline__ double beat_select(const double* cum, const int* flag, long long n, long long k, int lane) {
    unsigned long long res = 0;
    for (int bit = 63; bit >= 0; --bit) {
        const unsigned long long cand = res | (1ull << bit);
        long long c = 0;
        for (long long i = lane; i < n; i += kBeatWave) c += flag[i] && beat_key(cum[i]) < cand;
        if (beat_wave_sum_ll(c) <= k) res = cand;
    }
    return beat_unkey(res);
}

// grid = batch, block = kBeatWave (one wave)
template <class T> __global__ __launch_bounds__(kBeatWave) void beat_track_kernel(Args a) {
    __shared__ double ring[kBeatRing];
    __shared__ double pen[kBeatRing];
    __shared__ double sh_thr;
    const long long row = blockIdx.x, n = a.n;
    const int lane = (int)threadIdx.x;
    const T* ls = reinterpret_cast<const T*>(a.local) + row * n;
    double* cum = a.cum + row * n;
    int* bl = a.backlink + row * n;
    int* ord = a.order + row * n;
    unsigned char* out = a.out + row * n;
    for (long long i = lane; i < n; i += kBeatWave) out[i] = 0;
    if (a.dead[row]) return;
    const double ninf = -__builtin_inf();

    // (1) the first-beat threshold: 0.01 * max(localscore) in float64 (np.max hands a NaN on)
    double m = ninf;
    int has_nan = 0;
    for (long long i = lane; i < n; i += kBeatWave) {
        const double v = (double)ls[i];
        if (v != v) has_nan = 1;
        else m = v > m ? v : m;
    }
    m = beat_wave_max(m);
    const double thresh = beat_wave_ballot(has_nan) ? __builtin_nan("") : 0.01 * m;

    // (2) the recurrence
    const double tight = (double)a.tightness;
    const bool per_frame = a.bpm_mode == kPerFrame;
    const double* fpbp = per_frame ? a.fpb + row * n : a.fpb + row;
    double f = fpbp[0];
    int dmin = (int)rint(f / 2.0), dmax = 2 * (int)f;
    double logf = log(f);
    const bool fast = !per_frame && dmax <= kBeatRing;
    if (fast)
        for (int j = lane; j <= dmax - dmin; j += kBeatWave) {
            const double df = log((double)(dmin + j)) - logf;
            pen[j] = tight * (df * df);
        }
    __syncthreads();
    bool first = true;
    double si = (double)ls[0];
    for (long long i = 0; i < n; ++i) {
        const double si_next = i + 1 < n ? (double)ls[i + 1] : 0.0;  // (loaded a frame ahead: off the dependent chain)
        if (per_frame) {
            f = fpbp[i];
            dmin = (int)rint(f / 2.0);
            dmax = 2 * (int)f;
            logf = log(f);
        }
        const int dhi = dmax < i ? dmax : (int)i;  // loc >= 0
        double best = ninf;
        int bd = 0x7fffffff;
        for (int d = dmin + lane; d <= dhi; d += kBeatWave) {
            const long long loc = i - d;
            const double c = d <= kBeatRing ? ring[loc & (kBeatRing - 1)] : cum[loc];
            double p;
            if (fast) {
                p = pen[d - dmin];
            } else {
                const double df = log((double)d) - logf;
                p = tight * (df * df);
            }
            const double s = c - p;
            if (s > best) {  // strict: a lane keeps its smallest distance = largest loc on a tie
                best = s;
                bd = d;
            }
        }
        const double wbest = beat_wave_max(best);
        long long loc = -1;
        if (wbest > ninf) {
            const int mine = best == wbest;
            const unsigned long long eq = beat_wave_ballot(mine);
            int d;
            if ((eq & (eq - 1)) == 0) d = beat_wave_read(bd, __builtin_ffsll((long long)eq) - 1);
            else d = (int)-beat_wave_max_ll(mine ? -(long long)bd : -0x7fffffffLL);  // a tie across lanes: the smallest distance
            loc = i - d;
        }
        const double ci = loc >= 0 ? si + wbest : si;
        int link = -1;
        if (!(first && si < thresh)) {
            link = (int)loc;
            first = false;
        }
        if (lane == 0) {
            ring[i & (kBeatRing - 1)] = ci;
            cum[i] = ci;
            bl[i] = link;
        }
        si = si_next;
        __syncthreads();
    }

    // (3) the tail: the last local maximum of cum at or above half the median of cum over its local maxima (np.ma.median: the mean of the
    //     two middle values for an even count), else the last frame
    long long cnt = 0;
    for (long long i = lane; i < n; i += kBeatWave) {
        const int lm = beat_is_localmax(cum, i, n);
        ord[i] = lm;
        cnt += lm;
    }
    cnt = beat_wave_sum_ll(cnt);
    __syncthreads();
    double thr = 0.0;
    if (cnt > 0) {
        const long long k_lo = (cnt - 1) / 2, k_hi = cnt / 2;
        const double lo = beat_select(cum, ord, n, k_lo, lane);
        const double hi = k_hi == k_lo ? lo : beat_select(cum, ord, n, k_hi, lane);
        thr = 0.5 * ((cnt & 1) ? lo : (lo + hi) / 2.0);
    }
    long long tail = -1;
    for (long long i = lane; i < n; i += kBeatWave)
        if (ord[i] && cum[i] >= thr) tail = i;
    tail = beat_wave_max_ll(tail);
    if (tail < 0) tail = n - 1;
    __syncthreads();

    // (4) the walk along the back-links and the trim threshold, one lane
    if (lane == 0) {
        long long nb = 0, p = tail;
        for (long long step = 0; step < n && p >= 0; ++step) {
            out[p] = 1;
            ord[nb++] = (int)p;
            const long long q = bl[p];
            if (q >= p) break;  // (cannot happen; a wrong link ends the walk)
            p = q;
        }
        // np.convolve(localscore[beats], np.hanning(5))[2 : n + 2] with hanning(5) = [0, 0.5, 1, 0.5, 0]; 0.5 * rms of it
        double t2 = 0.0;
        if (a.trim) {
            const long long jend = n + 2 < nb + 4 ? n + 2 : nb + 4;
            double ss = 0.0;
            for (long long j = 2; j < jend; ++j) {
                double c = 0.0;
                for (int k = 1; k <= 3; ++k) {
                    const long long idx = j - k;
                    if (idx >= 0 && idx < nb) c += (k == 2 ? 1.0 : 0.5) * (double)ls[ord[nb - 1 - idx]];
                }
                ss += c * c;
            }
            t2 = 0.5 * sqrt(ss / (double)(jend - 2));
        }
        sh_thr = t2;
    }
    __syncthreads();

    // (5) the trim: every frame of the leading and of the trailing run with localscore <= threshold is cleared
    const double t2 = sh_thr;
    long long fk = n, lk = -1;
    for (long long i = lane; i < n; i += kBeatWave)
        if (!((double)ls[i] <= t2)) {
            if (i < fk) fk = i;
            lk = i;
        }
    fk = -beat_wave_max_ll(-fk);
    lk = beat_wave_max_ll(lk);
    for (long long i = lane; i < n; i += kBeatWave)
        if (i < fk || i > lk) out[i] = 0;
}

}  // namespace beat
}  // namespace lra

#pragma clang fp contract(fast)
