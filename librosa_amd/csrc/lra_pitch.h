// lra_pitch.h -- librosa.piptrack, pitch_tuning and estimate_tuning (librosa/core/pitch.py:28-366): the parabolic-interpolation pitch tracker
// on a resident magnitude spectrogram, the exact median of the peaks' magnitudes and the histogram of the tuning residuals.
// Self-contained so that tests/hostsim/pitchsim.cpp can run the same kernel bodies on the host (-DLRA_POSTSIM).
//
// S is addressed by (batch, bin, frame) strides; |.| is taken on load.  T = float or double.
//   piptrack_rows_kernel   bin_stride == 1 (what the STFT family writes, [b][t][pitch]).  Lanes run along the bins, a wave owns whole frames
//                          (a workgroup of kWaves waves takes kRowsF frames).  A frame's row is staged in the wave's LDS tile (kTile bins and
//                          one halo bin on either side) while its maximum is taken, and the stencil reads f - 1, f, f + 1 from the tile: a row
//                          of up to kTile bins is read from memory once.  A longer row goes tile by tile and, with ref = max, is staged twice
//                          (the maximum has to be known before the first peak test).
//   piptrack_cols_kernel   any other strides, meant for frame_stride == 1 (a C-contiguous (..., f, t) array).  One thread per frame, lanes
//                          along time, two walks over the bins (maximum, then the stencil on three rolling values).
// Both write every element of pitches / mags (zeros where there is no peak), or, as the kEmit variant, only the peaks with pitch > 0: frame i
// owns the slots [i * cap, (i + 1) * cap) of peak_pitch / peak_mag and peak_count[i] says how many it filled, in bin order.  Two adjacent
// bins are never both peaks (x[f] >= x[f + 1] and x[f + 1] > x[f] exclude each other), so cap = ceil(masked bins / 2) always suffices.
//   select_count_kernel / select_scan_kernel   radix select of the two middle order statistics of the emitted magnitudes on the
//                          order-preserving integer key of T, kDigitBits bits per pass: counts in an LDS histogram per workgroup, flushed
//                          by one integer atomic per non-empty bin; one small workgroup then narrows both ranks.  The last pass leaves
//                          thr = (lower + upper) / 2 in T (np.median) in the state block.
//   tuning_hist_kernel     residual = mod(bins_per_octave * log2(f / 27.5), 1), folded into [-0.5, 0.5), in T; np.histogram's bin by
//                          comparison with the host's float64 edge table (last bin closed); int64 counts, staged in LDS when the bins fit.
// Counts are integers and the selection is exact, so no result depends on the order in which waves arrive.  Every loop is bounded by a size
// or a constant.
#pragma once

#ifdef LRA_POSTSIM
#include <math.h>
#else
#include <hip/hip_runtime.h>
#endif

namespace lra {
namespace pitch {

constexpr int kRefMax = 0, kRefRow = 1, kRefScalar = 2;  // the LRA_PITCH_REF_* values of include/librosa_amd.h
constexpr int kNT = 256;        // threads of a workgroup (every kernel)
constexpr int kWaves = 4;       // waves of a workgroup
constexpr int kTile = 1088;     // bins a wave stages at a time: 1025 (n_fft 2048) and the tail of the last 64
constexpr int kRowsF = 16;      // frames per workgroup of piptrack_rows_kernel
constexpr int kColsF = kNT;     // frames per workgroup of piptrack_cols_kernel
constexpr int kDigitBits = 11;  // bits the radix select settles per pass
constexpr int kDigits = 1 << kDigitBits;
constexpr int kHistLds = 4096;  // histogram bins that are staged in LDS
constexpr int kPlainSeg = 4096; // slots per segment when a plain frequency array is walked (pitch_tuning)
constexpr int kSegLanes = 16;   // lanes that share a segment in the grid-stride kernels: a frame holds a handful of peaks, so a wave takes
constexpr int kSegsPerWave = 64 / kSegLanes;  // four segments per step
constexpr int kMaxGrid = 2048;  // workgroups of the grid-stride kernels (each flushes its partial counts once)
static_assert(kNT == 64 * kWaves && kRowsF % kWaves == 0 && kTile % 64 == 0 && kDigits % kNT == 0, "pitch kernel geometry");

struct Args {
    const void* s;  // T, element (b, f, t) at b * batch_stride + f * bin_stride + t * frame_stride
    long long batch_stride, bin_stride, frame_stride;
    int n_bins;
    long long n_frames;
    int lo, hi;            // the bins of the frequency mask: lo <= f < hi
    int ref_mode;          // kRef*
    double threshold;      // kRefMax: ref_value = (T)threshold * max_f S
    const double* ref_row; // kRefRow: ref_value[b * n_frames + t] (already multiplied by the threshold)
    double ref_scalar;     // kRefScalar: ref_value
    double sr, n_fft;      // pitches = (f + shift) * sr / n_fft in float64
    void* pitches;         // dense results, element (b, f, t) at b * out_batch_stride + f * out_bin_stride + t * out_frame_stride
    void* mags;
    long long out_batch_stride, out_bin_stride, out_frame_stride;
    void* peak_pitch;      // kEmit: T [batch * n_frames][cap]
    void* peak_mag;
    int* peak_count;       // kEmit: [batch * n_frames]
    int cap;
    long long tiles_per_clip;
};

struct SelectState {
    unsigned long long prefix[2];  // the key bits settled so far, of the lower and the upper middle element
    unsigned long long rank[2];    // their ranks among the elements that share the prefix
    unsigned long long total;      // number of emitted peaks
    double thr;                    // the median, as T in the first bytes
};

struct SelectArgs {
    const void* mag;       // T [n_segments][cap]
    const int* count;      // [n_segments]
    long long n_segments;
    int cap;
    unsigned long long* hist;  // [2][kDigits], zero on entry of every pass
    SelectState* state;
};

struct HistArgs {
    const void* freq;      // T [n_segments][cap]
    const void* mag;       // T, or null: no magnitude test
    const int* count;      // [n_segments], or null: every segment is full but the last (n_total elements in all)
    long long n_segments, n_total;
    int cap;
    const SelectState* state;  // with mag: only mag >= state->thr counts
    const double* edges;   // [n_hist + 1], np.linspace(-0.5, 0.5, n_hist + 1)
    int n_hist;
    double bins_per_octave;
    unsigned long long* out;   // [n_hist + 2], zero on entry: the counts, then the number of frequencies that entered the histogram's input
};

#ifdef LRA_POSTSIM
double pitch_shfl_xor(double v, int offset);     // the value of lane (lane ^ offset) of the same wave
unsigned long long pitch_ballot(int predicate);  // bit l: lane l's predicate
inline void pitch_add(unsigned* p, unsigned v) { *p += v; }
inline void pitch_add(unsigned long long* p, unsigned long long v) { *p += v; }
#else
__device__ __forceinline__ float pitch_shfl_xor(float v, int offset) { return __shfl_xor(v, offset, 64); }
__device__ __forceinline__ double pitch_shfl_xor(double v, int offset) { return __shfl_xor(v, offset, 64); }
__device__ __forceinline__ unsigned long long pitch_ballot(int predicate) { return __ballot(predicate); }
__device__ __forceinline__ void pitch_add(unsigned* p, unsigned v) { atomicAdd(p, v); }
__device__ __forceinline__ void pitch_add(unsigned long long* p, unsigned long long v) { atomicAdd(p, v); }
#endif

__device__ __forceinline__ float pitch_abs(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double pitch_abs(double v) { return __builtin_fabs(v); }
__device__ __forceinline__ float pitch_log2(float v) { return ::log2f(v); }
__device__ __forceinline__ double pitch_log2(double v) { return ::log2(v); }
__device__ __forceinline__ float pitch_trunc(float v) { return __builtin_truncf(v); }
__device__ __forceinline__ double pitch_trunc(double v) { return __builtin_trunc(v); }
// np.max: a NaN stays
template <class T> __device__ __forceinline__ T pitch_max(T m, T v) { return (v > m || v != v) ? v : m; }

// The reference value of frame (b, t) once the frame's maximum is known.
template <class T> __device__ __forceinline__ double pitch_ref(const Args& a, long long b, long long t, T frame_max) {
    if (a.ref_mode == kRefMax) return (double)((T)a.threshold * frame_max);
    if (a.ref_mode == kRefRow) return a.ref_row[b * a.n_frames + t];
    return a.ref_scalar;
}

// Bin f of a frame with its neighbours xm = S[f - 1], x0 = S[f], xp = S[f + 1] (whatever at the ends): true at a peak, with pitches and mags.
template <class T> __device__ __forceinline__ bool pitch_eval(const Args& a, int f, T xm, T x0, T xp, double ref, T& pitch, T& mag) {
    if (f < a.lo || f >= a.hi || f == 0) return false;
    const bool last = f == a.n_bins - 1;
    // util.localmax on S * (S > ref_value)
    const T tm = (double)xm > ref ? xm : (T)0, t0 = (double)x0 > ref ? x0 : (T)0, tp = (double)xp > ref ? xp : (T)0;
    if (!(t0 > tm) || !(last || t0 >= tp)) return false;
    T shift = (T)0, avg = x0 - xm;  // the last bin: no shift, one-sided gradient
    if (!last) {
        const T pa = xp + xm - (T)2 * x0;
        const T pb = (xp - xm) / (T)2;
        avg = pb;
        shift = pitch_abs(pb) >= pitch_abs(pa) ? (T)0 : -pb / pa;
    }
    const T dskew = (T)0.5 * avg * shift;
    mag = x0 + dskew;
    pitch = (T)(((double)f + (double)shift) * a.sr / a.n_fft);
    return true;
}

// grid = batch * tiles_per_clip (tiles of kRowsF frames), block = kNT; requires bin_stride == 1 (and, dense, out_bin_stride == 1)
template <class T, bool kEmit> __global__ __launch_bounds__(kNT) void piptrack_rows_kernel(Args a) {
    __shared__ T tiles[kWaves][kTile + 2];  // slot j holds bin f0 - 1 + j of the wave's frame
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long b = (long long)blockIdx.x / a.tiles_per_clip;
    const long long t0 = ((long long)blockIdx.x % a.tiles_per_clip) * kRowsF;
    const T* sb = reinterpret_cast<const T*>(a.s) + b * a.batch_stride;
    const int n_bins = a.n_bins;
    const int n_tiles = (n_bins + kTile - 1) / kTile;
    T* mine = tiles[wave];
    for (int i = 0; i < kRowsF / kWaves; ++i) {  // (every wave takes every step, so that the barriers are the workgroup's)
        const long long t = t0 + i * kWaves + wave;
        const bool live = t < a.n_frames;
        const T* row = sb + (live ? t : t0) * a.frame_stride;  // (a wave past the last frame repeats the tile's first and stores nothing)
        T m = (T)0;
        bool staged = false;
        if (a.ref_mode == kRefMax) {
            for (int bt = 0; bt < n_tiles; ++bt) {
                const int f0 = bt * kTile;
                __syncthreads();
                for (int j = lane; j < kTile + 2; j += 64) {
                    const int f = f0 - 1 + j;
                    const T v = (f >= 0 && f < n_bins) ? pitch_abs(row[f]) : (T)0;
                    mine[j] = v;
                    m = pitch_max<T>(m, v);
                }
            }
            for (int off = 32; off > 0; off >>= 1) m = pitch_max<T>(m, (T)pitch_shfl_xor(m, off));
            staged = n_tiles == 1;
        }
        const double ref = pitch_ref<T>(a, b, live ? t : t0, m);
        const long long frame = b * a.n_frames + t;
        T* po = reinterpret_cast<T*>(a.pitches) + b * a.out_batch_stride + t * a.out_frame_stride;
        T* mo = reinterpret_cast<T*>(a.mags) + b * a.out_batch_stride + t * a.out_frame_stride;
        int filled = 0;
        for (int bt = 0; bt < n_tiles; ++bt) {
            const int f0 = bt * kTile;
            const int width = n_bins - f0 < kTile ? n_bins - f0 : kTile;
            if (!staged) {
                __syncthreads();
                for (int j = lane; j < kTile + 2; j += 64) {
                    const int f = f0 - 1 + j;
                    mine[j] = (f >= 0 && f < n_bins) ? pitch_abs(row[f]) : (T)0;
                }
            }
            __syncthreads();
            // the bins of this tile that can hold a peak (dense: every bin is written)
            const int j_lo = kEmit ? (a.lo > f0 ? a.lo - f0 : 0) : 0;
            const int j_hi = kEmit ? (a.hi - f0 < width ? a.hi - f0 : width) : width;
            for (int j0 = j_lo - (j_lo & 63); j0 < j_hi; j0 += 64) {
                const int j = j0 + lane;
                T pitch = (T)0, mag = (T)0;
                bool peak = false;
                if (j < width) peak = pitch_eval<T>(a, f0 + j, mine[j], mine[j + 1], mine[j + 2], ref, pitch, mag);
                if (kEmit) {
                    const unsigned long long votes = pitch_ballot(peak && pitch > (T)0);
                    const int slot = filled + __builtin_popcountll(votes & ((1ull << lane) - 1ull));
                    if (live && peak && pitch > (T)0 && slot < a.cap) {
                        reinterpret_cast<T*>(a.peak_pitch)[frame * a.cap + slot] = pitch;
                        reinterpret_cast<T*>(a.peak_mag)[frame * a.cap + slot] = mag;
                    }
                    filled += __builtin_popcountll(votes);
                } else if (live && j < width) {
                    po[f0 + j] = peak ? pitch : (T)0;
                    mo[f0 + j] = peak ? mag : (T)0;
                }
            }
        }
        if (kEmit && live && lane == 0) a.peak_count[frame] = filled < a.cap ? filled : a.cap;
    }
}

// grid = batch * tiles_per_clip (tiles of kColsF frames), block = kNT; any strides
template <class T, bool kEmit> __global__ __launch_bounds__(kNT) void piptrack_cols_kernel(Args a) {
    const long long b = (long long)blockIdx.x / a.tiles_per_clip;
    const long long t = ((long long)blockIdx.x % a.tiles_per_clip) * kColsF + (long long)threadIdx.x;
    if (t >= a.n_frames) return;
    const T* sp = reinterpret_cast<const T*>(a.s) + b * a.batch_stride + t * a.frame_stride;
    const int n_bins = a.n_bins;
    T m = (T)0;
    if (a.ref_mode == kRefMax)
        for (int f = 0; f < n_bins; ++f) m = pitch_max<T>(m, pitch_abs(sp[(long long)f * a.bin_stride]));
    const double ref = pitch_ref<T>(a, b, t, m);
    const long long frame = b * a.n_frames + t;
    T* po = reinterpret_cast<T*>(a.pitches) + b * a.out_batch_stride + t * a.out_frame_stride;
    T* mo = reinterpret_cast<T*>(a.mags) + b * a.out_batch_stride + t * a.out_frame_stride;
    const int f_lo = kEmit ? (a.lo > 0 ? a.lo : 0) : 0;
    const int f_hi = kEmit ? (a.hi < n_bins ? a.hi : n_bins) : n_bins;
    int filled = 0;
    T xm = (T)0, x0 = (T)0, xp = (T)0;
    if (f_lo < f_hi) {
        xm = f_lo > 0 ? pitch_abs(sp[(long long)(f_lo - 1) * a.bin_stride]) : (T)0;
        x0 = pitch_abs(sp[(long long)f_lo * a.bin_stride]);
    }
    for (int f = f_lo; f < f_hi; ++f) {
        xp = f + 1 < n_bins ? pitch_abs(sp[(long long)(f + 1) * a.bin_stride]) : (T)0;
        T pitch = (T)0, mag = (T)0;
        const bool peak = pitch_eval<T>(a, f, xm, x0, xp, ref, pitch, mag);
        if (kEmit) {
            if (peak && pitch > (T)0 && filled < a.cap) {
                reinterpret_cast<T*>(a.peak_pitch)[frame * a.cap + filled] = pitch;
                reinterpret_cast<T*>(a.peak_mag)[frame * a.cap + filled] = mag;
                ++filled;
            }
        } else {
            po[(long long)f * a.out_bin_stride] = peak ? pitch : (T)0;
            mo[(long long)f * a.out_bin_stride] = peak ? mag : (T)0;
        }
        xm = x0;
        x0 = xp;
    }
    if (kEmit) a.peak_count[frame] = filled;
}

// ---- the exact median of the emitted magnitudes --------------------------------------------------------------------------------------------
template <class T> struct Key;
template <> struct Key<float> {
    static constexpr int bits = 32;
    static __device__ __forceinline__ unsigned long long of(float v) {
        const unsigned u = __builtin_bit_cast(unsigned, v);
        return (u & 0x80000000u) ? (unsigned)~u : (u | 0x80000000u);
    }
    static __device__ __forceinline__ float back(unsigned long long k) {
        const unsigned u = (unsigned)k;
        return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7fffffffu) : (unsigned)~u);
    }
};
template <> struct Key<double> {
    static constexpr int bits = 64;
    static __device__ __forceinline__ unsigned long long of(double v) {
        const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
        return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    }
    static __device__ __forceinline__ double back(unsigned long long k) {
        return __builtin_bit_cast(double, (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
    }
};
template <class T> struct Passes { static constexpr int value = (Key<T>::bits + kDigitBits - 1) / kDigitBits; };
// pass p settles the bits [shift, shift + width) of the key, from the top
template <class T> __device__ __forceinline__ int pass_shift(int p) { const int s = Key<T>::bits - kDigitBits * (p + 1); return s > 0 ? s : 0; }
template <class T> __device__ __forceinline__ int pass_width(int p) { return p + 1 < Passes<T>::value ? kDigitBits : Key<T>::bits - kDigitBits * (Passes<T>::value - 1); }

// grid <= kMaxGrid, block = kNT: kSegLanes lanes take a whole segment, a wave kSegsPerWave segments per step
template <class T> __global__ __launch_bounds__(kNT) void select_count_kernel(SelectArgs a, int pass) {
    __shared__ unsigned lh[2 * kDigits];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 2 * kDigits; i += kNT) lh[i] = 0u;
    __syncthreads();
    const int shift = pass_shift<T>(pass), width = pass_width<T>(pass);
    const unsigned long long p0 = a.state->prefix[0], p1 = a.state->prefix[1];
    const T* mag = reinterpret_cast<const T*>(a.mag);
    const long long step = (long long)gridDim.x * kWaves * kSegsPerWave;
    for (long long seg = ((long long)blockIdx.x * kWaves + wave) * kSegsPerWave + lane / kSegLanes; seg < a.n_segments; seg += step) {
        const int n = a.count[seg] < a.cap ? a.count[seg] : a.cap;
        for (int j = lane % kSegLanes; j < n; j += kSegLanes) {
            const unsigned long long k = Key<T>::of(mag[seg * a.cap + j]);
            const unsigned long long top = pass == 0 ? 0ull : k >> (shift + width);
            const unsigned digit = (unsigned)(k >> shift) & ((1u << width) - 1u);
            if (pass == 0 || top == p0) pitch_add(&lh[digit], 1u);
            if (pass == 0 || top == p1) pitch_add(&lh[kDigits + digit], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < 2 * kDigits; i += kNT)
        if (lh[i]) pitch_add(&a.hist[i], (unsigned long long)lh[i]);
}

// grid = 1, block = kNT: narrows both ranks by the pass's digit, clears the histogram, and after the last pass leaves the median
template <class T> __global__ __launch_bounds__(kNT) void select_scan_kernel(SelectArgs a, int pass) {
    constexpr int kPer = kDigits / kNT;
    __shared__ unsigned long long part[2][kNT];
    const int tid = (int)threadIdx.x;
    for (int r = 0; r < 2; ++r) {
        unsigned long long s = 0;
        for (int i = 0; i < kPer; ++i) s += a.hist[r * kDigits + tid * kPer + i];
        part[r][tid] = s;
    }
    __syncthreads();
    if (tid < 2) {
        const int r = tid;
        unsigned long long total = 0;
        for (int i = 0; i < kNT; ++i) total += part[r][i];
        unsigned long long rank = a.state->rank[r];
        if (pass == 0) {
            rank = r == 0 ? (total ? (total - 1) / 2 : 0) : total / 2;
            if (r == 0) a.state->total = total;
        }
        unsigned long long below = 0;
        int chunk = 0;
        bool found = false;
        for (int i = 0; i < kNT; ++i) {
            const unsigned long long c = part[r][i];
            if (!found && rank < below + c) {
                found = true;
                chunk = i;
            }
            if (!found) below += c;
        }
        int digit = chunk * kPer;
        bool hit = false;
        for (int i = 0; i < kPer; ++i) {
            const unsigned long long c = a.hist[r * kDigits + chunk * kPer + i];
            if (found && !hit && rank < below + c) {
                hit = true;
                digit = chunk * kPer + i;
            }
            if (found && !hit) below += c;
        }
        a.state->rank[r] = rank - (found ? below : 0);
        a.state->prefix[r] = ((pass == 0 ? 0ull : a.state->prefix[r]) << pass_width<T>(pass)) | (unsigned long long)digit;
    }
    __syncthreads();
    for (int i = tid; i < 2 * kDigits; i += kNT) a.hist[i] = 0ull;
    if (pass == Passes<T>::value - 1 && tid == 0) {
        // np.median: the mean of the two middle values in T (the value itself for an odd count); 0 when there is no peak
        const T lower = Key<T>::back(a.state->prefix[0]), upper = Key<T>::back(a.state->prefix[1]);
        a.state->thr = 0.0;
        *reinterpret_cast<T*>(&a.state->thr) = a.state->total ? (lower + upper) / (T)2 : (T)0;
    }
}

// ---- residuals and their histogram ----------------------------------------------------------------------------------------------------------
// np.histogram's bin of x among edges[0 .. n]: edges[i] <= x < edges[i + 1], the last bin closed; -1 outside (and for a NaN)
__device__ __forceinline__ int hist_bin(const double* edges, int n, double x) {
    if (!(x >= edges[0]) || !(x <= edges[n])) return -1;
    // the edges are equally spaced up to rounding: the computed bin is right or off by one, which two comparisons settle; whatever they
    // cannot confirm goes through the search below
    int g = (int)((x - edges[0]) / (edges[n] - edges[0]) * (double)n);
    g = g < 0 ? 0 : (g > n - 1 ? n - 1 : g);
    if (g > 0 && x < edges[g]) --g;
    else if (g < n - 1 && x >= edges[g + 1]) ++g;
    if (x >= edges[g] && (x < edges[g + 1] || g == n - 1)) return g;
    int lo = 0, hi = n;  // edges[lo] <= x, and x < edges[hi] or hi == n
    for (int it = 0; it < 32; ++it) {
        if (hi - lo <= 1) break;
        const int mid = lo + (hi - lo) / 2;
        if (x >= edges[mid]) lo = mid;
        else hi = mid;
    }
    return lo;
}

// grid <= kMaxGrid, block = kNT: kSegLanes lanes take a whole segment, a wave kSegsPerWave segments per step
template <class T> __global__ __launch_bounds__(kNT) void tuning_hist_kernel(HistArgs a) {
    __shared__ unsigned lh[kHistLds + 1];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool staged = a.n_hist <= kHistLds;
    for (int i = tid; i < kHistLds + 1; i += kNT) lh[i] = 0u;
    __syncthreads();
    const T* freq = reinterpret_cast<const T*>(a.freq);
    const T* mag = reinterpret_cast<const T*>(a.mag);
    const T thr = mag ? *reinterpret_cast<const T*>(&a.state->thr) : (T)0;
    const long long step = (long long)gridDim.x * kWaves * kSegsPerWave;
    for (long long seg = ((long long)blockIdx.x * kWaves + wave) * kSegsPerWave + lane / kSegLanes; seg < a.n_segments; seg += step) {
        const long long rest = a.n_total - seg * a.cap;
        int n = a.count ? a.count[seg] : (rest < a.cap ? (int)rest : a.cap);
        n = n < a.cap ? n : a.cap;
        for (int j = lane % kSegLanes; j < n; j += kSegLanes) {
            const T f = freq[seg * a.cap + j];
            if (!(f > (T)0)) continue;
            if (mag && !(mag[seg * a.cap + j] >= thr)) continue;
            pitch_add(&lh[kHistLds], 1u);
            T r = (T)a.bins_per_octave * pitch_log2(f / (T)27.5);
            r = r - pitch_trunc(r);            // fmod(r, 1), exact
            if (r < (T)0) r += (T)1;           // np.mod takes the divisor's sign
            if (r >= (T)0.5) r -= (T)1;
            const int bin = hist_bin(a.edges, a.n_hist, (double)r);
            if (bin < 0) continue;
            if (staged) pitch_add(&lh[bin], 1u);
            else pitch_add(&a.out[bin], 1ull);
        }
    }
    __syncthreads();
    if (staged)
        for (int i = tid; i < a.n_hist; i += kNT)
            if (lh[i]) pitch_add(&a.out[i], (unsigned long long)lh[i]);
    if (tid == 0 && lh[kHistLds]) pitch_add(&a.out[a.n_hist], (unsigned long long)lh[kHistLds]);
}

}  // namespace pitch
}  // namespace lra
