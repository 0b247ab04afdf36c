// lra_onset.h -- spectral-flux onset strength: librosa.onset.onset_strength / onset_strength_multi (librosa/onset.py:217-367, 445-645).
// Self-contained so that tests/hostsim/onsetsim.cpp can run the same kernel bodies on host threads (-DLRA_POSTSIM).
//
//   S      = power_to_db(|mel|)                         (DB: evaluated on the fly from the power spectrogram, lra_db.h; else S as given)
//   ref    = S | maximum_filter1d(S, max_size, axis=bands, mode="reflect") | the caller's ref
//   env    = max(0, S[..., lag:] - ref[..., :-lag])     (np.maximum: a NaN propagates)
//   odf    = util.sync(env, channels, aggregate, axis=bands), then `pad` zeros on the left, trimmed to n_out frames
//   detrend: scipy.signal.lfilter([1, -1], [1, -0.99], odf, axis=time) from a zero state, in float64
//
// The input is the [item][band][frame] layout the mel kernel writes.  One thread per output frame, lanes along time: every band row is
// read with coalesced wave loads (as dct_rows_kernel does), the flux of a band is formed in registers, and only the aggregated rows
// are written.  The band max filter runs on the raw power before the decibel step (the step is monotone, so the max of the decibels is
// the decibel of the max, exactly), so no dB or ref array is ever materialised.  Mean / sum / max / min accumulate in registers;
// the median stages a channel's flux values of each frame in LDS (one column per lane) and selects the middle order statistics with a
// radix select on the IEEE bit patterns (the rectified flux is +0, positive or NaN, and non-negative floats order like their bits).
#pragma once

#ifndef LRA_POSTSIM
#include <hip/hip_runtime.h>
#endif

#include "lra_db.h"
#include "lra_pcen.h"  // PcenOps: one rounding per operation

#ifdef LRA_POSTSIM
#define LRA_ONSET_DYN_LDS(T, name) T* name = reinterpret_cast<T*>(g_postsim_dyn_lds)
#else
#define LRA_ONSET_DYN_LDS(T, name)                                            \
    extern __shared__ __attribute__((aligned(16))) unsigned char lra_onset_lds[]; \
    T* name = reinterpret_cast<T*>(lra_onset_lds)
#endif

namespace lra {

// aggregation codes (the LRA_ONSET_* values of include/librosa_amd.h)
constexpr int kOnsetNone = 0, kOnsetMean = 1, kOnsetSum = 2, kOnsetMax = 3, kOnsetMin = 4, kOnsetMedian = 5, kOnsetRows = 6;

template <class T> struct OnsetArgs {
    const T* S;          // [batch][n_bands][n_frames]: power (DB) or the spectrogram as given; kOnsetRows: finished envelope rows
    const T* ref;        // [batch][n_bands][n_frames] caller's reference, used as given, or nullptr
    T* out;              // [batch][n_rows][n_out], n_rows = n_ch (aggregates) or n_bands (kOnsetNone / kOnsetRows)
    const int* ch_off;   // [n_ch + 1] offsets into ch_band (aggregates only), or nullptr: one channel of every band in order (channels=None)
    const int* ch_band;  // band indices of the channels, channel after channel (nullptr with ch_off)
    long long batch, n_frames, pad, n_out;
    int n_bands, lag, max_size, n_ch;
    DbArgs<T> db;        // DB only: amin, ref_scalar, per-item maxima of |S|, top_db
};

template <class T> struct OnsetBits;
template <> struct OnsetBits<float> {
    using U = unsigned int;
    static constexpr int kBits = 31;  // the sign bit is always clear
};
template <> struct OnsetBits<double> {
    using U = unsigned long long;
    static constexpr int kBits = 63;
};

// np.maximum(0.0, d): negatives (and -0) become +0, a NaN propagates
template <class T> __device__ __forceinline__ T onset_rectify(T d) { return d > (T)0 ? d : (d != d ? d : (T)0); }

// the per-band value of one frame: the rectified flux, or (kOnsetRows) the input row itself
template <class T, bool DB, int AGG> struct OnsetSrc {
    const T* s;  // this item's [n_bands][n_frames]
    const T* r;  // this item's caller reference or nullptr
    long long nf;
    int nb, lag, max_size;
    T amin, ref_db, floor_db;

    __device__ __forceinline__ T mag(T v) const { return DB ? (v < (T)0 ? -v : v) : v; }  // power_to_db(np.abs(S))
    __device__ __forceinline__ T conv(T v) const {
        if (!DB) return v;
        const T db = db_of<T>(v, amin, ref_db);
        return db > floor_db ? db : floor_db;
    }
    __device__ __forceinline__ T at(int m, long long e) const {
        const T* __restrict__ row = s + (long long)m * nf;
        if (AGG == kOnsetRows) return row[e];
        const T cur = conv(mag(row[e + lag]));
        T prev;
        if (r) {
            prev = r[(long long)m * nf + e];
        } else if (max_size == 1) {
            prev = conv(mag(row[e]));
        } else {
            // scipy.ndimage.maximum_filter1d, mode="reflect" (d c b a | a b c d | d c b a), origin 0: bands m - size/2 .. m - size/2 + size - 1
            const int period = 2 * nb;
            int idx = (m - max_size / 2) % period;
            if (idx < 0) idx += period;
            T v = mag(s[(long long)(idx < nb ? idx : period - 1 - idx) * nf + e]);
            for (int j = 1; j < max_size; ++j) {
                idx = idx + 1 == period ? 0 : idx + 1;
                const T c = mag(s[(long long)(idx < nb ? idx : period - 1 - idx) * nf + e]);
                v = c > v ? c : v;
            }
            prev = conv(v);
        }
        return onset_rectify<T>(cur - prev);
    }
};

template <class T, bool DB, int AGG> __device__ __forceinline__ OnsetSrc<T, DB, AGG> onset_src(const OnsetArgs<T>& a, long long b) {
    OnsetSrc<T, DB, AGG> src;
    src.s = a.S + b * (long long)a.n_bands * a.n_frames;
    src.r = a.ref ? a.ref + b * (long long)a.n_bands * a.n_frames : nullptr;
    src.nf = a.n_frames;
    src.nb = a.n_bands;
    src.lag = a.lag;
    src.max_size = a.max_size;
    src.amin = a.db.amin;
    src.ref_db = (T)0;
    src.floor_db = (T)-INFINITY;
    if (DB) db_item_constants<T>(a.db, b, false, src.ref_db, src.floor_db);
    return src;
}

// frames of the un-padded envelope: S[..., lag:] has n_frames - lag of them (none when lag >= n_frames); kOnsetRows: the rows as given
template <class T, int AGG> __device__ __forceinline__ long long onset_env_frames(const OnsetArgs<T>& a) {
    if (AGG == kOnsetRows) return a.n_frames;
    return a.n_frames > a.lag ? a.n_frames - a.lag : 0;
}

// mean / sum / max / min over channels, or (kOnsetNone, kOnsetRows) every band as its own row.  grid: batch x ceil(n_out / 256), block 256.
template <class T, bool DB, int AGG>
__global__ __launch_bounds__(256) void onset_flux_kernel(OnsetArgs<T> a) {
    const long long tblocks = (a.n_out + 255) / 256;
    const long long b = blockIdx.x / tblocks;
    const long long j = (blockIdx.x % tblocks) * 256 + threadIdx.x;
    const OnsetSrc<T, DB, AGG> src = onset_src<T, DB, AGG>(a, b);
    if (j >= a.n_out) return;
    const long long e = j - a.pad;  // the padding is written here: no host np.pad or copy follows
    const bool live = e >= 0 && e < onset_env_frames<T, AGG>(a);
    if (AGG == kOnsetNone || AGG == kOnsetRows) {
        T* __restrict__ o = a.out + b * (long long)a.n_bands * a.n_out + j;
        for (int m = 0; m < a.n_bands; ++m) o[(long long)m * a.n_out] = live ? src.at(m, e) : (T)0;
        return;
    }
    T* __restrict__ o = a.out + b * (long long)a.n_ch * a.n_out + j;
    for (int c = 0; c < a.n_ch; ++c) {
        const int lo = a.ch_off ? a.ch_off[c] : 0, hi = a.ch_off ? a.ch_off[c + 1] : a.n_bands;  // uniform: scalar loads
        T acc = (T)0;
        if (live) {
            if (AGG == kOnsetMean || AGG == kOnsetSum) {
                // np.add.reduce over the band axis: one band after the other, in the channel's order
                for (int k = lo; k < hi; ++k) acc += src.at(a.ch_band ? a.ch_band[k] : k, e);
                // np.mean divides by the count as an integer scalar: in float64, rounded once to T (an empty channel gives 0 / 0 = NaN)
                if (AGG == kOnsetMean) acc = (T)((double)acc / (double)(hi - lo));
            } else if (hi > lo) {  // (the host rejects empty channels for max / min, as np.max raises on them)
                acc = src.at(a.ch_band ? a.ch_band[lo] : lo, e);
                for (int k = lo + 1; k < hi; ++k) {
                    const T v = src.at(a.ch_band ? a.ch_band[k] : k, e);
                    const bool take = AGG == kOnsetMax ? v > acc : v < acc;
                    acc = (take || v != v) ? v : acc;  // NaN wins and stays, as np.max / np.min propagate it
                }
            }
        }
        o[(long long)c * a.n_out] = acc;
    }
}

// k-th smallest (0-based) of n non-negative keys held in an LDS column (stride `ld`): radix select from the top bit down, kBits passes over
// the column, the same passes for every lane (no data-dependent branches)
template <class T> __device__ __forceinline__ typename OnsetBits<T>::U onset_select(const T* col, int ld, int n, int k) {
    using U = typename OnsetBits<T>::U;
    U prefix = 0;
    for (int bit = OnsetBits<T>::kBits - 1; bit >= 0; --bit) {
        const U want = prefix >> bit;  // the decided high bits, this bit 0
        int cnt = 0;
        for (int i = 0; i < n; ++i) cnt += (__builtin_bit_cast(U, col[(long long)i * ld]) >> bit) == want;
        if (k >= cnt) {
            k -= cnt;
            prefix |= (U)1 << bit;
        }
    }
    return prefix;
}

// np.median over each channel's bands: exact (the mean of the two middle values for an even count).  One thread per output frame; a
// workgroup of `fb` frames stages, channel by channel, its flux values in LDS [max channel size][fb] (the host sizes fb to the LDS).
// frames per workgroup of the median kernel (host side, shared by the launch and the simulator): a whole wave while the LDS tile
// [max_ch_bands][frames] stays within 64 KiB, fewer for very wide channels, down to one frame (the 160 KiB of a CU); 0 when even that does not fit
inline int onset_median_frames(int max_ch_bands, size_t elem) {
    int fb = 64;
    while (fb > 1 && (size_t)max_ch_bands * fb * elem > 64 * 1024) fb /= 2;
    return (size_t)max_ch_bands * fb * elem <= 160 * 1024 ? fb : 0;
}

template <class T, bool DB>
__global__ __launch_bounds__(64) void onset_median_kernel(OnsetArgs<T> a) {
    using U = typename OnsetBits<T>::U;
    LRA_ONSET_DYN_LDS(T, lds);
    const int fb = (int)blockDim.x;
    const long long tblocks = (a.n_out + fb - 1) / fb;
    const long long b = blockIdx.x / tblocks;
    const long long j = (blockIdx.x % tblocks) * fb + threadIdx.x;
    const OnsetSrc<T, DB, kOnsetMedian> src = onset_src<T, DB, kOnsetMedian>(a, b);
    if (j >= a.n_out) return;
    const long long e = j - a.pad;
    const bool live = e >= 0 && e < onset_env_frames<T, kOnsetMedian>(a);
    T* col = lds + threadIdx.x;  // this lane's column: lanes on consecutive words, no bank conflicts
    T* __restrict__ o = a.out + b * (long long)a.n_ch * a.n_out + j;
    for (int c = 0; c < a.n_ch; ++c) {
        const int lo = a.ch_off ? a.ch_off[c] : 0, n = a.ch_off ? a.ch_off[c + 1] - lo : a.n_bands;
        T res = (T)0;
        if (live) {
            bool nan = n == 0;  // np.median of an empty slice is NaN
            for (int k = 0; k < n; ++k) {
                const T v = src.at(a.ch_band ? a.ch_band[lo + k] : lo + k, e);
                nan |= v != v;
                col[(long long)k * fb] = v;
            }
            if (nan) {
                res = (T)NAN;  // np.median returns NaN when the slice holds one
            } else {
                const int k1 = (n - 1) / 2;
                const U v1 = onset_select<T>(col, fb, n, k1);
                U v2 = v1;
                if (n % 2 == 0) {  // the next order statistic: v1 again when it repeats, else the smallest key above it
                    int le = 0;
                    U above = ~(U)0;
                    for (int i = 0; i < n; ++i) {
                        const U key = __builtin_bit_cast(U, col[(long long)i * fb]);
                        le += key <= v1;
                        above = key > v1 && key < above ? key : above;
                    }
                    v2 = le > k1 + 1 ? v1 : above;
                }
                const T x1 = __builtin_bit_cast(T, v1), x2 = __builtin_bit_cast(T, v2);
                // np.mean of the middle slice: the sum in T, divided by the count in float64, rounded once
                res = n % 2 ? x1 : (T)((double)(x1 + x2) / 2.0);
            }
        }
        o[(long long)c * a.n_out] = res;
    }
}

// detrend: scipy.signal.lfilter([1, -1], [1, -0.99], x, axis=-1) from a zero state on independent rows of float64 (the reference's
// result is float64 whatever the envelope's type).  Transposed direct form II as scipy evaluates it, one rounding per operation:
// y = z + 1 x;  z = x (-1) - y (-0.99).  The tiling of pcen_kernel: one wave owns kOnsetDetrendRows rows, a tile of kOnsetDetrendTile frames
// is loaded with lanes along time into LDS, the first kOnsetDetrendRows lanes run the recurrence in place, the tile is stored with lanes along
// time again.  The padded leading zeros keep the state at zero, so filtering the padded row equals the reference's pad-then-filter.
constexpr int kOnsetDetrendRows = 16, kOnsetDetrendTile = 64;

template <class T> __global__ __launch_bounds__(64) void onset_detrend_kernel(const T* __restrict__ x, double* __restrict__ out, long long rows, long long n) {
    using R = PcenOps;
    __shared__ double sm[kOnsetDetrendRows][kOnsetDetrendTile + 1];  // row pitch 65 doubles: the recurrence lanes hit distinct banks
    const int lane = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * kOnsetDetrendRows;
    const int nrows = (int)(rows - row0 < kOnsetDetrendRows ? rows - row0 : kOnsetDetrendRows);
    double z = 0;
    for (long long f0 = 0; f0 < n; f0 += kOnsetDetrendTile) {
        const int nf = (int)(n - f0 < kOnsetDetrendTile ? n - f0 : kOnsetDetrendTile);
        if (lane < nf)
            for (int r = 0; r < nrows; ++r) sm[r][lane] = (double)x[(row0 + r) * n + f0 + lane];
        __syncthreads();
        if (lane < nrows) {
            for (int i = 0; i < nf; ++i) {
                const double xi = sm[lane][i];
                const double y = R::add(z, R::mul(1.0, xi));
                z = R::sub(R::mul(xi, -1.0), R::mul(y, -0.99));
                sm[lane][i] = y;
            }
        }
        __syncthreads();
        if (lane < nf)
            for (int r = 0; r < nrows; ++r) out[(row0 + r) * n + f0 + lane] = sm[r][lane];
        __syncthreads();
    }
}

}  // namespace lra
