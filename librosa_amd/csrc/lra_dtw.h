// lra_dtw.h -- librosa.sequence.dtw and dtw_backtracking (librosa/sequence.py:185-694): the cost matrix, the accumulated cost matrix and the
// warping path, all on the device.
// Self-contained so that tests/hostsim/dtwsim.cpp can run the same kernel bodies on host fibres (-DLRA_POSTSIM).
//
//   D[n][m] starts at +inf; at C[0][0] for (0, 0); at C[0][m] for the whole first row under subseq.  Then, for the steps i = 0 .. n_steps - 1
//   in table order:
//       cur_C = w_mul[i] * C[n][m];  cur_C += w_add[i];  cost = D[n - s0[i]][m - s1[i]] + cur_C;  if (cost < D[n][m]) { D[n][m] = cost; steps[n][m] = i; }
//   with D = +inf outside the matrix and steps[n][m] = 0 where no candidate improved the cell.  Every candidate is one float64 multiplication and
//   two float64 additions, each rounded on its own, and a strict comparison: hipcc would contract w_mul * C + w_add into one fused multiply-add,
//   which rounds once and gives other bits than the reference, so the functions that form candidates carry `#pragma clang fp contract(off)`
//   (the pragma, not the __dmul_rn / __dadd_rn intrinsics: the same source then serves the host simulator).
//
//   dtw_cost        C[n][m] = metric(X[:, n], Y[:, m]) in float64 from float32 or float64 features [K][N], [K][M]: a workgroup per 32 x 32 tile of
//                   C, the tiles of X and Y in LDS 32 features at a time, the features summed in ascending order.  cosine of a zero vector is NaN
//                   (0 / 0), as scipy's.  A NaN raises kFlagNan in one word.
//   dtw_prepare     a given C of float32, float64, int32, int64 or uint8 -> float64 (exactly, but for int64 beyond 2^53), and the same NaN flag.
//                   A float64 C is only checked: the accumulation reads it where it lies.
//   dtw_accumulate  The matrix is cut into square tiles of edge T.  All tiles of one tile anti-diagonal run in one launch, one workgroup of one
//                   wave per tile; the host issues the ceil(N / T) + ceil(M / T) - 1 launches in stream order, so no workgroup waits on
//                   another.  The tile's C (band applied as a predicate) is loaded as coalesced rows into LDS; D lives in LDS with a halo of max_0
//                   rows above and max_1 columns to the left, read from the global D of earlier launches (+inf outside the matrix).  Lane r owns
//                   local row r; the wave sweeps the 2T - 1 local anti-diagonals with a wave-level fence between them (no workgroup barrier:
//                   there is one wave), every predecessor an LDS read.  D and the step indices (uint8) leave as coalesced rows at the end.
//   dtw_widen       the uint8 step indices -> int32, only where the caller wants `steps`.
//   dtw_backtrack   one workgroup: under subseq the first argmin of D[-1, :] by a reduction that prefers the lower index, else (N - 1, M - 1) or a
//                   given start; then one thread follows the reference's loop (:610-640), including the break when an index goes negative.
//                   The path holds at most N + M - 1 pairs, as no step is (0, 0).  Serves dtw_backtracking on int32 steps as well.
// Everything that scales with N * M is indexed in 64 bits.
#pragma once

#ifndef LRA_POSTSIM
#include <hip/hip_runtime.h>
#endif

#include <cstdint>

#ifdef LRA_POSTSIM
#define LRA_DTW_DYN_LDS(ptr) char* ptr = reinterpret_cast<char*>(g_postsim_dyn_lds)
#else
#define LRA_DTW_DYN_LDS(ptr) extern __shared__ __align__(16) char lra_dtw_lds[]; char* ptr = lra_dtw_lds
#endif

namespace lra {
namespace dtw {

constexpr int kMaxSteps = 16;  // LRA_DTW_MAX_STEPS: rows of the step table, the three defaults included
constexpr int kMaxStep = 8;    // LRA_DTW_MAX_STEP: the largest step component (the halo of the smallest tile)
constexpr int kDefaultTile = 64;
constexpr int kEuclidean = 0, kSqeuclidean = 1, kCityblock = 2, kCosine = 3;                                   // the LRA_DTW_* metrics
constexpr int kF32 = 0, kF64 = 1, kI32 = 2, kI64 = 3, kU8 = 4;                                                 // the types dtw_prepare reads
constexpr int kFlagNan = 1, kFlagEndInf = 2, kFlagRowInf = 4, kFlagNotOrigin = 8, kFlagBadStep = 16;           // the LRA_DTW_FLAG_* bits
constexpr long long kStartEnd = -1, kStartArgmin = -2;                                                        // LRA_DTW_START_*
constexpr int kLdsMax = 160 * 1024;
constexpr int kAccNT = 64;  // one wave per tile; no tile is wider than a wave
constexpr int kLoadRows = 32;
constexpr int kCostTile = 32, kCostK = 32, kCostNT = 256;
constexpr int kPrepNT = 256, kBackNT = 256;

constexpr bool tile_ok(int tile) { return tile == 8 || tile == 16 || tile == 32 || tile == 64; }

// what an accumulate launch looks like for a tile edge (0: the library's choice) and the largest step components
struct Geometry {
    int tile;
    int d_rows;    // rows of the LDS D: tile + max_0
    int d_stride;  // doubles per row of it: tile + max_1, rounded up to even so that the lanes of a local anti-diagonal (r, d - r) are d_stride - 1
                   // doubles apart, an odd number: no two of 32 lanes share a pair of banks
    int off_c;     // byte offset of the C tile [tile][tile] (tile - 1 is odd already)
    int off_s;     // byte offset of the step indices [tile][tile] uint8
    int lds;       // bytes of dynamic LDS
};
constexpr Geometry geometry(int tile, int max0, int max1) {
    Geometry g{};
    g.tile = tile ? tile : kDefaultTile;
    g.d_rows = g.tile + max0;
    g.d_stride = (g.tile + max1 + 1) / 2 * 2;
    g.off_c = g.d_rows * g.d_stride * 8;
    g.off_s = g.off_c + g.tile * g.tile * 8;
    g.lds = g.off_s + g.tile * g.tile;
    return g;
}

// the tiles of tile anti-diagonal `diag` of a tiles_n x tiles_m grid: tile rows first .. first + count - 1 (tile column diag - row)
struct DiagTiles {
    long long first, count;
};
constexpr DiagTiles diag_tiles(long long diag, long long tiles_n, long long tiles_m) {
    const long long first = diag - (tiles_m - 1) > 0 ? diag - (tiles_m - 1) : 0;
    const long long last = diag < tiles_n - 1 ? diag : tiles_n - 1;
    return DiagTiles{first, last - first + 1};
}

struct StepTable {
    int n, max0, max1;
    int s0[kMaxSteps], s1[kMaxSteps];
    double w_add[kMaxSteps], w_mul[kMaxSteps];
};

struct CostArgs {
    const void* X;  // [K][N]
    const void* Y;  // [K][M]
    int f64;
    int metric;
    long long K, N, M;
    double* C;      // [N][M]
    int* flags;
};

struct PrepArgs {
    const void* in;
    int dtype;
    long long count;
    double* out;  // null: check only
    int* flags;
};

struct AccArgs {
    const double* C;  // [N][M]
    long long N, M;
    StepTable st;
    int subseq;
    int band;                   // C[n][m] reads as +inf where m - n >= band_hi or m - n <= band_lo
    long long band_lo, band_hi;
    double* D;                  // [N][M]
    uint8_t* steps;             // [N][M]
    long long diag, tiles_n, tiles_m;
    Geometry g;
};

struct WidenArgs {
    const uint8_t* in;
    long long count;
    int* out;
};

struct BackArgs {
    const double* D;    // null: no checks of D (dtw_backtracking)
    const void* steps;  // [N][M] uint8, or int32 (steps_i32)
    int steps_i32;
    long long N, M;
    StepTable st;
    int subseq;
    long long start;    // a column, kStartEnd or kStartArgmin (needs D)
    long long* path;    // [cap][2]
    long long cap;
    long long* length;
    int* status;
};

#ifdef LRA_POSTSIM
void dtw_wave_sync();
void dtw_flag_or(int* word, int bits);
#else
// the LDS stores of the wave's lanes before this point are seen by its loads after it (one wave: no workgroup barrier is needed)
__device__ __forceinline__ void dtw_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void dtw_flag_or(int* word, int bits) { atomicOr(word, bits); }
#endif

__device__ __forceinline__ double dtw_inf() { return __builtin_huge_val(); }
__device__ __forceinline__ bool dtw_isinf(double v) { return v == dtw_inf() || v == -dtw_inf(); }

// np.argmin's order: the first NaN wins; otherwise the smaller value, the lower index on a tie; an index < 0: nothing there
__device__ __forceinline__ bool dtw_argmin_better(double v, long long i, double bv, long long bi) {
    if (i < 0) return false;
    if (bi < 0) return true;
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v < bv || (v == bv && i < bi);
}

__device__ __forceinline__ double dtw_feature(const void* p, int f64, long long at) {
    return f64 ? reinterpret_cast<const double*>(p)[at] : (double)reinterpret_cast<const float*>(p)[at];
}

// The metric body, shared with the neighbour search (lra_knn.h): one feature (x, y) added to the running sums in ascending feature order, every
// product and sum rounded on its own (contraction off), so that the sums are those of a NumPy model bit for bit.  cost_body below keeps its own
// statements: the compiler contracts some of them into fused multiply-adds, its results have shipped with those bits, and routing it through
// this function changes them ...
__device__ __forceinline__ void dtw_metric_add(int metric, double x, double y, double& acc, double& xx, double& yy) {
#pragma clang fp contract(off)
    if (metric == kCosine) {
        acc += x * y;
        xx += x * x;
        yy += y * y;
    } else if (metric == kCityblock) {
        acc += __builtin_fabs(x - y);
    } else {
        const double d = x - y;
        acc += d * d;
    }
}

// ... and the distance of the finished sums (cost_body's too: nothing here can be contracted)
__device__ __forceinline__ double dtw_metric_finish(int metric, double acc, double xx, double yy) {
    double c = acc;
    if (metric == kEuclidean) {
        c = sqrt(c);
    } else if (metric == kCosine) {
        // scipy's cdist: the cosine clipped to [-1, 1], then 1 - cosine; 0 / 0 is NaN and stays NaN
        double cs = acc / (sqrt(xx) * sqrt(yy));
        if (__builtin_fabs(cs) > 1.0) cs = cs < 0.0 ? -1.0 : 1.0;
        c = 1.0 - cs;
    }
    return c;
}

// grid = ceil(N / kCostTile) * ceil(M / kCostTile) workgroups of kCostNT threads; thread (ty, tx) forms C[n0 + ty + 8 i][m0 + tx], i < 4
__device__ __forceinline__ void cost_body(const CostArgs& a) {
    __shared__ double xs[kCostK][kCostTile];
    __shared__ double ys[kCostK][kCostTile];
    constexpr int kPer = kCostTile * kCostTile / kCostNT, kRows = kCostNT / kCostTile;
    const long long tiles_m = (a.M + kCostTile - 1) / kCostTile;
    const long long n0 = ((long long)blockIdx.x / tiles_m) * kCostTile, m0 = ((long long)blockIdx.x % tiles_m) * kCostTile;
    const int tid = (int)threadIdx.x, tx = tid % kCostTile, ty = tid / kCostTile;
    double acc[kPer], xx[kPer], yy[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) acc[i] = xx[i] = yy[i] = 0.0;
    for (long long k0 = 0; k0 < a.K; k0 += kCostK) {
        const int kk = a.K - k0 < kCostK ? (int)(a.K - k0) : kCostK;
        for (int q = tid; q < kk * kCostTile; q += kCostNT) {
            const int k = q / kCostTile, j = q % kCostTile;
            xs[k][j] = n0 + j < a.N ? dtw_feature(a.X, a.f64, (k0 + k) * a.N + n0 + j) : 0.0;
            ys[k][j] = m0 + j < a.M ? dtw_feature(a.Y, a.f64, (k0 + k) * a.M + m0 + j) : 0.0;
        }
        __syncthreads();
        for (int k = 0; k < kk; ++k) {
            const double y = ys[k][tx];
#pragma unroll
            for (int i = 0; i < kPer; ++i) {
                const double x = xs[k][ty + kRows * i];
                if (a.metric == kCosine) {
                    acc[i] += x * y;
                    xx[i] += x * x;
                    yy[i] += y * y;
                } else if (a.metric == kCityblock) {
                    acc[i] += __builtin_fabs(x - y);
                } else {
                    const double d = x - y;
                    acc[i] += d * d;
                }
            }
        }
        __syncthreads();
    }
    int flags = 0;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const long long n = n0 + ty + kRows * i, m = m0 + tx;
        if (n >= a.N || m >= a.M) continue;
        const double c = dtw_metric_finish(a.metric, acc[i], xx[i], yy[i]);
        if (c != c) flags |= kFlagNan;
        a.C[n * a.M + m] = c;
    }
    if (flags) dtw_flag_or(a.flags, flags);
}

__device__ __forceinline__ double dtw_given(const void* p, int dtype, long long at) {
    switch (dtype) {
        case kF32: return (double)reinterpret_cast<const float*>(p)[at];
        case kF64: return reinterpret_cast<const double*>(p)[at];
        case kI32: return (double)reinterpret_cast<const int32_t*>(p)[at];
        case kI64: return (double)reinterpret_cast<const int64_t*>(p)[at];
        default: return (double)reinterpret_cast<const uint8_t*>(p)[at];
    }
}

// grid = ceil(count / kPrepNT) workgroups of kPrepNT threads
__device__ __forceinline__ void prepare_body(const PrepArgs& a) {
    const long long at = (long long)blockIdx.x * kPrepNT + (long long)threadIdx.x;
    if (at >= a.count) return;
    const double v = dtw_given(a.in, a.dtype, at);
    if (a.out) a.out[at] = v;
    if (v != v) dtw_flag_or(a.flags, kFlagNan);
}

// grid = ceil(count / kPrepNT) workgroups of kPrepNT threads
__device__ __forceinline__ void widen_body(const WidenArgs& a) {
    const long long at = (long long)blockIdx.x * kPrepNT + (long long)threadIdx.x;
    if (at < a.count) a.out[at] = (int)a.in[at];
}

// grid = diag_tiles(diag, tiles_n, tiles_m).count workgroups of kAccNT threads; dynamic LDS = g.lds.  NS: the rows of the step table when they
// are the three defaults' number (the loop over candidates unrolled, their LDS reads issued together), 0: any number
template <int NS>
__device__ __forceinline__ void accumulate_body(const AccArgs& a) {
#pragma clang fp contract(off)
    LRA_DTW_DYN_LDS(lds);
    const Geometry& g = a.g;
    const int T = g.tile, ds = g.d_stride, max0 = a.st.max0, max1 = a.st.max1, lane = (int)threadIdx.x;
    double* Dl = reinterpret_cast<double*>(lds);
    double* Cl = reinterpret_cast<double*>(lds + g.off_c);
    uint8_t* Sl = reinterpret_cast<uint8_t*>(lds + g.off_s);
    const long long ti = diag_tiles(a.diag, a.tiles_n, a.tiles_m).first + (long long)blockIdx.x, tj = a.diag - ti;
    const long long n0 = ti * T, m0 = tj * T, N = a.N, M = a.M;
    const int rows = N - n0 < T ? (int)(N - n0) : T, cols = M - m0 < T ? (int)(M - m0) : T;
    // the tile's C, row by row (a row is at most one element per lane), the band as a predicate; kLoadRows loads are in flight before the first
    // is stored (one row per round trip to memory would cost more than the sweep itself)
    for (int r0 = 0; r0 < rows; r0 += kLoadRows) {
        double v[kLoadRows];
#pragma unroll
        for (int i = 0; i < kLoadRows; ++i) {
            const long long gn = n0 + r0 + i, gm = m0 + lane, dm = gm - gn;
            const bool masked = a.band && (dm >= a.band_hi || dm <= a.band_lo);
            v[i] = r0 + i < rows && lane < cols && !masked ? a.C[gn * M + gm] : dtw_inf();
        }
#pragma unroll
        for (int i = 0; i < kLoadRows; ++i)
            if (r0 + i < rows && lane < cols) Cl[(r0 + i) * T + lane] = v[i];
    }
    // the halo: max0 rows above (with the corner), max1 columns to the left, from the D of earlier launches; +inf outside the matrix
    for (int hr = 0; hr < max0; ++hr)
        for (int hc = lane; hc < max1 + cols; hc += kAccNT) {
            const long long gn = n0 - max0 + hr, gm = m0 - max1 + hc;
            Dl[hr * ds + hc] = gn >= 0 && gm >= 0 ? a.D[gn * M + gm] : dtw_inf();
        }
    for (int q = lane; q < rows * max1; q += kAccNT) {
        const int r = q / max1, hc = q % max1;
        const long long gn = n0 + r, gm = m0 - max1 + hc;
        Dl[(max0 + r) * ds + hc] = gm >= 0 ? a.D[gn * M + gm] : dtw_inf();
    }
    dtw_wave_sync();
    const int n_steps = NS ? NS : a.st.n;
    const bool live = lane < rows;
    const long long gn = n0 + lane;
    double* drow = Dl + (lane + max0) * ds + max1;  // (the lane's own row of D, at local column 0)
    for (int d = 0; d < rows + cols - 1; ++d) {
        const int c = d - lane;
        if (live && c >= 0 && c < cols) {
            const double cv = Cl[lane * T + c];
            double best = (gn == 0 && (a.subseq || m0 + c == 0)) ? cv : dtw_inf();
            int bs = 0;
            if constexpr (NS > 0) {
                double prev[NS];
#pragma unroll
                for (int i = 0; i < NS; ++i) prev[i] = drow[c - a.st.s0[i] * ds - a.st.s1[i]];
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    double cur = a.st.w_mul[i] * cv;
                    cur += a.st.w_add[i];
                    const double cost = prev[i] + cur;
                    if (cost < best) { best = cost; bs = i; }
                }
            } else {
                for (int i = 0; i < n_steps; ++i) {
                    const double prev = drow[c - a.st.s0[i] * ds - a.st.s1[i]];
                    double cur = a.st.w_mul[i] * cv;
                    cur += a.st.w_add[i];
                    const double cost = prev + cur;
                    if (cost < best) { best = cost; bs = i; }
                }
            }
            drow[c] = best;
            Sl[lane * T + c] = (uint8_t)bs;
        }
        dtw_wave_sync();
    }
    for (int r = 0; r < rows; ++r)
        for (int c = lane; c < cols; c += kAccNT) {
            const long long at = (n0 + r) * M + m0 + c;
            a.D[at] = Dl[(r + max0) * ds + max1 + c];
            a.steps[at] = Sl[r * T + c];
        }
}

// one workgroup of kBackNT threads
__device__ __forceinline__ void backtrack_body(const BackArgs& a) {
    __shared__ double red_v[kBackNT];
    __shared__ long long red_i[kBackNT];
    __shared__ int red_f[kBackNT];
    const int tid = (int)threadIdx.x;
    const long long N = a.N, M = a.M;
    if (a.start == kStartArgmin) {
        const double* last = a.D + (N - 1) * M;
        double bv = 0.0;
        long long bi = -1;
        int finite = 0;
        for (long long j = tid; j < M; j += kBackNT) {
            const double v = last[j];
            if (!dtw_isinf(v)) finite = 1;
            if (dtw_argmin_better(v, j, bv, bi)) { bv = v; bi = j; }
        }
        red_v[tid] = bv;
        red_i[tid] = bi;
        red_f[tid] = finite;
    }
    __syncthreads();
    if (tid != 0) return;
    int status = 0;
    long long m = a.start == kStartEnd ? M - 1 : a.start;
    if (a.start == kStartArgmin) {
        double bv = red_v[0];
        long long bi = red_i[0];
        int finite = red_f[0];
        for (int i = 1; i < kBackNT; ++i) {
            finite |= red_f[i];
            if (dtw_argmin_better(red_v[i], red_i[i], bv, bi)) { bv = red_v[i]; bi = red_i[i]; }
        }
        m = bi;
        if (!finite) status |= kFlagRowInf;
    } else if (a.D && !a.subseq && dtw_isinf(a.D[(N - 1) * M + M - 1])) {
        status |= kFlagEndInf;
    }
    long long len = 0;
    if (!status) {
        long long n = N - 1;
        a.path[0] = n;
        a.path[1] = m;
        len = 1;
        long long ln = n, lm = m;
        while (a.subseq ? n > 0 : (n != 0 || m != 0)) {
            const long long at = n * M + m;
            const int s = a.steps_i32 ? reinterpret_cast<const int*>(a.steps)[at] : (int)reinterpret_cast<const uint8_t*>(a.steps)[at];
            if (s < 0 || s >= a.st.n) {
                status |= kFlagBadStep;
                break;
            }
            n -= a.st.s0[s];
            m -= a.st.s1[s];
            if (n < 0 || m < 0) break;  // ran off the side of the matrix (:634)
            if (len >= a.cap) {         // (cannot happen while no step is (0, 0): every step lowers n + m)
                status |= kFlagBadStep;
                break;
            }
            a.path[2 * len] = n;
            a.path[2 * len + 1] = m;
            ++len;
            ln = n;
            lm = m;
        }
        if (!a.subseq && (ln != 0 || lm != 0)) status |= kFlagNotOrigin;
    }
    *a.length = len;
    *a.status = status;
}

// (plain functions, not templates: defined where LRA_DTW_KERNELS says so -- lra_dtw_inst.hip and the simulator -- and nowhere else)
#if defined(LRA_DTW_KERNELS) || defined(LRA_POSTSIM)
__global__ __launch_bounds__(kCostNT) void dtw_cost(CostArgs a) { cost_body(a); }
__global__ __launch_bounds__(kPrepNT) void dtw_prepare(PrepArgs a) { prepare_body(a); }
__global__ __launch_bounds__(kPrepNT) void dtw_widen(WidenArgs a) { widen_body(a); }
__global__ __launch_bounds__(kAccNT) void dtw_accumulate(AccArgs a) { accumulate_body<3>(a); }
__global__ __launch_bounds__(kAccNT) void dtw_accumulate_any(AccArgs a) { accumulate_body<0>(a); }
__global__ __launch_bounds__(kBackNT) void dtw_backtrack(BackArgs a) { backtrack_body(a); }
#endif

}  // namespace dtw
}  // namespace lra
