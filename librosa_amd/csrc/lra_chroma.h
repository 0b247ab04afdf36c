// lra_chroma.h -- chroma features: the dense projection raw[c][t] = sum_f W[c][f] X[f][t] of librosa.feature.chroma_stft / chroma_cqt
// (librosa/feature/spectral.py:1285-1293, 1407-1421), chroma_cqt's threshold and util.normalize(axis=-2, fill=None)
// (librosa/util/utils.py:959-1011) in one launch: the spectrogram is read once, only the n_chroma rows are written.
// Self-contained so that tests/hostsim/chromasim.cpp can run the same kernel bodies on the host (-DLRA_POSTSIM).
//
// The bank is dense (every weight of filters.chroma is non-zero in float32), so there are no bands to exploit: the kernels are a stream of X
// with kRows dot products per frame.  X is addressed by (batch, bin, frame) strides; out is [batch][n_chroma][n_frames].  T = float or double.
//   chroma_rows_kernel   bin_stride == 1 (what the power STFT writes, [b][t][pitch]).  A workgroup of kWaves waves takes kTileF frames.  The
//                        weights of kRows rows are staged in LDS (kBinTile bins at a time: once per workgroup and row chunk when the row of
//                        bins fits, else once per pass).  Lanes run along the bins; a wave carries kFr frames at once, so one LDS read of a
//                        weight feeds kFr multiply-adds.  The kFr x kRows partial sums of the 64 lanes are added by a reduce-scatter (every
//                        step halves the values a lane holds: 51 exchanges instead of 288) and land in an LDS tile [row][frame]; one thread
//                        per frame applies the threshold, raises the flag and accumulates the frame's length in float64; all threads then
//                        divide and store, frames along the lanes.
//   chroma_cols_kernel   any other strides, meant for frame_stride == 1 (a C-contiguous (..., f, t) array).  One thread per frame, lanes along
//                        time, kRows accumulators in registers, the weights wave-uniform.
// More than kRows rows: the rows go in chunks of kRows, each chunk a pass over X; the chunks' raw values are stored, the length is carried, and
// a last pass re-reads what the same thread stored and divides.
// The order of every sum depends on the bin and row index alone, so a clip alone gives the bits of that clip in a batch.
// Every loop is bounded by n_bins, n_chroma or a constant.
#pragma once

#ifndef LRA_POSTSIM
#include <hip/hip_runtime.h>
#endif

namespace lra {
namespace chroma {

constexpr int kNormNone = 0, kNormL1 = 1, kNormL2 = 2, kNormInf = 3;  // the LRA_CHROMA_NORM_* values of include/librosa_amd.h
constexpr int kNT = 256;      // threads of a workgroup (both kernels)
constexpr int kWaves = 4;     // waves of a workgroup
constexpr int kFr = 4;        // frames a wave carries at once (chroma_rows_kernel)
constexpr int kRows = 12;     // rows of W per chunk
constexpr int kPass = kWaves * kFr;  // frames a workgroup takes per pass
constexpr int kTileF = 64;    // frames per workgroup of chroma_rows_kernel
constexpr int kColsF = kNT;   // frames per workgroup of chroma_cols_kernel
constexpr int kTileBytes = 52224;  // LDS bytes of the staged weights: kRows x 1088 floats (1025 bins and the tail of the last 64) or x 544 doubles
static_assert(kNT == 64 * kWaves && kTileF % kPass == 0 && (kFr * kRows) % 16 == 0, "chroma kernel geometry");

template <class T> struct BinTile { static constexpr int value = kTileBytes / (kRows * (int)sizeof(T)); };

struct Args {
    const void* x;  // T, element (b, f, t) at b * batch_stride + f * bin_stride + t * frame_stride
    long long batch_stride, bin_stride, frame_stride;
    int n_bins;
    long long n_frames;
    const void* w;  // [n_chroma][n_bins] T
    int n_chroma;
    int norm;       // kNorm*
    int has_thr;    // raw < thr -> 0 before the normalisation
    double thr;
    void* out;      // [batch][n_chroma][n_frames] T
    int* flag;      // zeroed by the caller; set to 1 when some raw value (after the threshold) is not finite
    long long tiles_per_clip;
};

template <class T> struct Tiny;
template <> struct Tiny<float> { static constexpr double value = 1.17549435082228750797e-38; };
template <> struct Tiny<double> { static constexpr double value = 2.2250738585072014e-308; };

#ifdef LRA_POSTSIM
double chroma_shfl_xor(double v, int offset);  // the value of lane (lane ^ offset) of the same wave
#else
__device__ __forceinline__ float chroma_shfl_xor(float v, int offset) { return __shfl_xor(v, offset, 64); }
__device__ __forceinline__ double chroma_shfl_xor(double v, int offset) { return __shfl_xor(v, offset, 64); }
#endif
template <class T> __device__ __forceinline__ T chroma_xchg(T v, int offset) { return (T)chroma_shfl_xor(v, offset); }

// One step of the reduce-scatter: of the 2 H values in a[], a lane whose bit `offset` is clear keeps the sums of the first H, its partner those
// of the other H.
template <class T, int H> __device__ __forceinline__ void chroma_halve(T* a, int lane, int offset) {
    const bool hi = (lane & offset) != 0;
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const T send = hi ? a[i] : a[i + H];
        const T keep = hi ? a[i + H] : a[i];
        a[i] = keep + chroma_xchg<T>(send, offset);
    }
}

// threshold, flag and the frame's length contribution of one raw value (float64 magnitudes, librosa/util/utils.py:972-993)
template <class T> __device__ __forceinline__ T chroma_admit(T v, const Args& a, double& len) {
    if (a.has_thr && v < (T)a.thr) v = (T)0;
    const double m = v < (T)0 ? -(double)v : (double)v;
    if (!(m <= 1.7976931348623157e308)) *a.flag = 1;  // NaN or infinite
    if (a.norm == kNormInf) len = m > len ? m : len;  // (np.max hands a NaN on; the flag has then been raised anyway)
    else if (a.norm == kNormL1) len += m;
    else if (a.norm == kNormL2) len += m * m;
    return v;
}

template <class T> __device__ __forceinline__ double chroma_length(double len, int norm) {
    if (norm == kNormL2) len = __builtin_sqrt(len);
    if (norm == kNormNone || len < Tiny<T>::value) len = 1.0;  // a frame below `tiny` is left as it is
    return len;
}

// one division in float64, rounded to T (S / length with a float64 length, :1010)
template <class T> __device__ __forceinline__ T chroma_scale(T v, double len, int norm) { return norm == kNormNone ? v : (T)((double)v / len); }

// grid = batch * tiles_per_clip (tiles of kTileF frames), block = kNT; requires bin_stride == 1
template <class T> __global__ __launch_bounds__(kNT) void chroma_rows_kernel(Args a) {
    constexpr int kBT = BinTile<T>::value;
    constexpr int kV = kFr * kRows;
    __shared__ T wt[kRows * kBT];
    __shared__ T tile[kRows * kTileF];
    __shared__ double lens[kTileF];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long b = (long long)blockIdx.x / a.tiles_per_clip;
    const long long t0 = ((long long)blockIdx.x % a.tiles_per_clip) * kTileF;
    const int nt = (int)(a.n_frames - t0 < kTileF ? a.n_frames - t0 : kTileF);
    const T* xb = reinterpret_cast<const T*>(a.x) + b * a.batch_stride;
    const T* w = reinterpret_cast<const T*>(a.w);
    T* ob = reinterpret_cast<T*>(a.out) + b * (long long)a.n_chroma * a.n_frames;
    const int n_bins = a.n_bins;
    const int n_chunks = (a.n_chroma + kRows - 1) / kRows;
    const int n_btiles = (n_bins + kBT - 1) / kBT;
    double len = 0.0;  // of frame t0 + tid (threads below kTileF)
    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        const int c0 = chunk * kRows;
        const int nr = a.n_chroma - c0 < kRows ? a.n_chroma - c0 : kRows;
        for (int pass = 0; pass * kPass < nt; ++pass) {
            const int fbase = pass * kPass + wave * kFr;  // the wave's first frame, tile-relative
            T acc[kV];
#pragma unroll
            for (int v = 0; v < kV; ++v) acc[v] = (T)0;
            const T* xr[kFr];  // (a frame past the tile's last reads the tile's first instead: its sums are never used)
#pragma unroll
            for (int fr = 0; fr < kFr; ++fr) xr[fr] = xb + (t0 + (fbase + fr < nt ? fbase + fr : 0)) * a.frame_stride;
            for (int bt = 0; bt < n_btiles; ++bt) {
                const int f0 = bt * kBT;
                const int width = n_bins - f0 < kBT ? n_bins - f0 : kBT;
                if (n_btiles > 1 || pass == 0) {
                    __syncthreads();  // every wave is done with the weights staged before
                    for (int f = tid; f < kBT; f += kNT) {  // kRows independent loads per step; rows and bins past the end are staged as zeros
                        const T* wc = w + (long long)c0 * n_bins + f0 + (f < width ? f : 0);
                        T wv[kRows];
#pragma unroll
                        for (int r = 0; r < kRows; ++r) wv[r] = wc[(long long)(r < nr ? r : 0) * n_bins];
#pragma unroll
                        for (int r = 0; r < kRows; ++r) wt[r * kBT + f] = (r < nr && f < width) ? wv[r] : (T)0;
                    }
                    __syncthreads();
                }
#pragma unroll 4
                for (int f = lane; f < width; f += 64) {
                    T xv[kFr];
#pragma unroll
                    for (int fr = 0; fr < kFr; ++fr) xv[fr] = xr[fr][f0 + f];
#pragma unroll
                    for (int r = 0; r < kRows; ++r) {
                        const T wv = wt[r * kBT + f];
#pragma unroll
                        for (int fr = 0; fr < kFr; ++fr) acc[fr * kRows + r] += wv * xv[fr];
                    }
                }
            }
            // 64 lanes x kV partial sums -> kV sums: after the four halvings a lane holds kV / 16 values, starting at value `first`
            chroma_halve<T, kV / 2>(acc, lane, 32);
            chroma_halve<T, kV / 4>(acc, lane, 16);
            chroma_halve<T, kV / 8>(acc, lane, 8);
            chroma_halve<T, kV / 16>(acc, lane, 4);
            const int first = (kV / 2) * ((lane >> 5) & 1) + (kV / 4) * ((lane >> 4) & 1) + (kV / 8) * ((lane >> 3) & 1) + (kV / 16) * ((lane >> 2) & 1);
#pragma unroll
            for (int i = 0; i < kV / 16; ++i) {
                T s = acc[i];
                s += chroma_xchg<T>(s, 2);
                s += chroma_xchg<T>(s, 1);
                const int v = first + i, fr = v / kRows, r = v - fr * kRows;
                if ((lane & 3) == 0) tile[r * kTileF + fbase + fr] = s;
            }
        }
        __syncthreads();
        if (tid < nt) {
            for (int r = 0; r < nr; ++r) tile[r * kTileF + tid] = chroma_admit<T>(tile[r * kTileF + tid], a, len);
            if (n_chunks == 1) lens[tid] = chroma_length<T>(len, a.norm);
        }
        __syncthreads();
        for (int i = tid; i < kRows * kTileF; i += kNT) {
            const int r = i / kTileF, t = i - r * kTileF;
            if (r < nr && t < nt) {
                const T v = tile[i];
                ob[(long long)(c0 + r) * a.n_frames + t0 + t] = n_chunks == 1 ? chroma_scale<T>(v, lens[t], a.norm) : v;
            }
        }
    }
    if (n_chunks > 1 && a.norm != kNormNone) {
        __syncthreads();
        if (tid < nt) lens[tid] = chroma_length<T>(len, a.norm);
        __syncthreads();
        for (int chunk = 0; chunk < n_chunks; ++chunk) {  // the same thread re-reads what it stored
            const int c0 = chunk * kRows;
            const int nr = a.n_chroma - c0 < kRows ? a.n_chroma - c0 : kRows;
            for (int i = tid; i < kRows * kTileF; i += kNT) {
                const int r = i / kTileF, t = i - r * kTileF;
                if (r < nr && t < nt) {
                    T* p = ob + (long long)(c0 + r) * a.n_frames + t0 + t;
                    *p = chroma_scale<T>(*p, lens[t], a.norm);
                }
            }
        }
    }
}

// grid = batch * tiles_per_clip (tiles of kColsF frames), block = kNT; any strides
template <class T> __global__ __launch_bounds__(kNT) void chroma_cols_kernel(Args a) {
    const long long b = (long long)blockIdx.x / a.tiles_per_clip;
    const long long t = ((long long)blockIdx.x % a.tiles_per_clip) * kColsF + (long long)threadIdx.x;
    if (t >= a.n_frames) return;
    const T* xp = reinterpret_cast<const T*>(a.x) + b * a.batch_stride + t * a.frame_stride;
    const T* w = reinterpret_cast<const T*>(a.w);
    T* op = reinterpret_cast<T*>(a.out) + b * (long long)a.n_chroma * a.n_frames + t;
    const int n_bins = a.n_bins;
    const int n_chunks = (a.n_chroma + kRows - 1) / kRows;
    double len = 0.0;
    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        const int c0 = chunk * kRows;
        const int nr = a.n_chroma - c0 < kRows ? a.n_chroma - c0 : kRows;
        T acc[kRows];
        const T* wr[kRows];
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            acc[r] = (T)0;
            wr[r] = w + (long long)(r < nr ? c0 + r : c0) * n_bins;  // (rows past the last repeat the chunk's first and are not stored)
        }
        for (int f = 0; f < n_bins; ++f) {
            const T xv = xp[(long long)f * a.bin_stride];
#pragma unroll
            for (int r = 0; r < kRows; ++r) acc[r] += wr[r][f] * xv;
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r)
            if (r < nr) acc[r] = chroma_admit<T>(acc[r], a, len);
        const double ln = n_chunks == 1 ? chroma_length<T>(len, a.norm) : 1.0;
#pragma unroll
        for (int r = 0; r < kRows; ++r)
            if (r < nr) op[(long long)(c0 + r) * a.n_frames] = n_chunks == 1 ? chroma_scale<T>(acc[r], ln, a.norm) : acc[r];
    }
    if (n_chunks > 1 && a.norm != kNormNone) {
        const double ln = chroma_length<T>(len, a.norm);
        for (int c = 0; c < a.n_chroma; ++c) {  // the same thread re-reads what it stored
            T* p = op + (long long)c * a.n_frames;
            *p = chroma_scale<T>(*p, ln, a.norm);
        }
    }
}

}  // namespace chroma
}  // namespace lra
