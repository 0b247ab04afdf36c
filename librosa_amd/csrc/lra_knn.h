// lra_knn.h -- the neighbour graphs of librosa.segment.cross_similarity and recurrence_matrix (librosa/segment.py:67-357, :361-706, and
// __affinity_bandwidth :1332-1437): the k nearest candidate frames of every query frame, selected without the [n][m] distance matrix, and the
// reference's sparse or dense result made of them, all on the device.
// Self-contained (with lra_dtw.h, whose metric body it shares) so that tests/hostsim/knnsim.cpp can run the same kernel bodies on host fibres
// (-DLRA_POSTSIM).
//
//   Query frame i (a column of Q [d][n]) keeps the k smallest (distance, index) pairs among its candidates j (columns of R [d][m]): every j
//   outside the band |i - j| < width (width 0: no band), and, with skip_zero, every j whose distance is not exactly 0.  Pairs are ordered by
//   distance, an exact tie by the lower index; a NaN distance is larger than every number.  The k smallest of a total order are one set, so the
//   result does not depend on the order in which candidates are met, nor on the geometry.
//
//   knn_select     A workgroup of kNT threads owns `rows` query frames and sweeps the candidates in tiles of `tile` frames.  The tile of
//                  distances is formed in float64 by dtw_metric_add / dtw_metric_finish (lra_dtw.h: every operation rounded on its own), kFeat features at a
//                  time through LDS, and left in LDS.  Then wave w owns the rows w, w + kWaves, ...: per 64 candidates one ballot of "is a
//                  candidate and beats the row's threshold", the set bits walked in order.  A row's list lives in LDS unsorted, with its largest
//                  pair (the threshold) and that pair's slot in registers, the same in every lane; a candidate that beats the threshold takes the
//                  slot, and the wave finds the new largest pair (each lane over its share of the list, then a butterfly of six lane exchanges).
//                  Until the list is full every candidate is appended.  Nothing of size n * m is written; the lists leave as (count, index,
//                  distance) per row.
//   knn_sort_rows  a workgroup per row: the list by ascending index (a rank sort in LDS; the indices of a row are distinct).
//   knn_mutual     one thread per list entry: keep[i][e] = not (drop_zero and distance == 0) and (not sym or i is in row j's list), a binary
//                  search of the sorted row j.
//   knn_bandwidth  a workgroup per row: the kept distances (and a 0 for the self link, where it is stored) sorted ascending; dist_to_k = the
//                  min(bandwidth_k, count)-th smallest, avg = the mean of those first ones summed in ascending order; an empty row gives NaN,
//                  raises kStatusRowEmpty and leaves the lowest such row.
//   knn_median     one workgroup: np.nanmedian(dist_to_k) by an exact radix select on the floats' integer keys, 8 bits a pass, for the one or
//                  two middle ranks; kStatusEmptyGraph where no entry is finite.
//   knn_bw_check   (bandwidth <= 0).any() of a bandwidth matrix -> kStatusNonPositive.
//   knn_count, knn_scan, knn_emit   the stored entries per row (the self link included), their exclusive sum (indptr), and the entries
//                  themselves: indices / data compacted in index order (the CSR arrays of the graph = the CSC arrays of the transposed
//                  result), or a scatter into the zero-filled dense result [m][n].  knn_value is the entry: 1, the distance, or
//                  exp(distance / -bandwidth) (knn_affinity) with the bandwidth of the entry (knn_entry_bandwidth: the six modes and a matrix).
//   knn_dense      where every candidate is kept: the transposed result [m][n] straight from the metric body, 32 x 32 tiles as dtw_cost.
// Everything that scales with n * k or n * m is indexed in 64 bits.
#pragma once

#ifndef LRA_POSTSIM
#include <hip/hip_runtime.h>
#endif

#include <cstdint>

#include "lra_dtw.h"

#ifdef LRA_POSTSIM
#define LRA_KNN_DYN_LDS(ptr) char* ptr = reinterpret_cast<char*>(g_postsim_dyn_lds)
#else
#define LRA_KNN_DYN_LDS(ptr) extern __shared__ __align__(16) char lra_knn_lds[]; char* ptr = lra_knn_lds
#endif

namespace lra {
namespace knn {

constexpr int kNT = 256, kWave = 64, kWaves = kNT / kWave;
constexpr int kFeat = 16;           // features staged in LDS at a time
constexpr int kPer = 8;             // distances of a tile per thread at the most: rows * tile <= kNT * kPer
constexpr int kMaxK = 2048;         // LRA_KNN_MAX_K: the longest list a row keeps
constexpr int kLdsMax = 64 * 1024;  // the dynamic LDS a workgroup takes at the most
constexpr int kDefaultRows = 4, kDefaultTile = 128;   // one row per wave: the selection is a chain of dependent steps per row, so rows are spread over as many waves as there are
constexpr int kConnectivity = 0, kDistance = 1, kAffinity = 2;                                           // LRA_KNN_* modes
constexpr int kBwScalar = 0, kBwMeanK = 1, kBwGmeanK = 2, kBwMeanKAvg = 3, kBwGmeanKAvg = 4, kBwMeanKAvgPair = 5, kBwMatrix = 6;   // LRA_KNN_BW_*
constexpr int kStatusEmptyGraph = 1, kStatusRowEmpty = 2, kStatusNonPositive = 4;                        // LRA_KNN_STATUS_*
constexpr int kWorkBytes = 64;      // LRA_KNN_WORK_BYTES: status word, first empty row, the scalar bandwidth, the entry count
constexpr int kSortNT = 256, kRowNT = 256, kMedNT = 256, kDenseTile = 32, kDenseNT = 256;

constexpr bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
constexpr int kMaxRows = 16;
constexpr bool rows_ok(int rows) { return pow2(rows) && rows <= kMaxRows; }
constexpr bool tile_ok(int tile) { return pow2(tile) && tile >= 4 && tile <= 1024; }

// what a select launch looks like for (rows, tile), 0: the library's choice, and lists of k pairs
struct Geometry {
    int rows, tile, k;
    int off_y;      // byte offset of the candidates' features [kFeat][tile] (the queries' [kFeat][rows] come first)
    int off_t;      // ... of the distance tile [rows][tile]
    int off_ld;     // ... of the lists' distances [rows][k]
    int off_li;     // ... of the lists' indices [rows][k]
    int lds;        // bytes of dynamic LDS; 0: not served
};
constexpr Geometry layout(int rows, int tile, int k) {
    Geometry g{};
    g.rows = rows;
    g.tile = tile;
    g.k = k;
    g.off_y = kFeat * rows * 8;
    g.off_t = g.off_y + kFeat * tile * 8;
    g.off_ld = g.off_t + rows * tile * 8;
    g.off_li = g.off_ld + rows * k * 8;
    g.lds = (g.off_li + rows * k * 4 + 15) / 16 * 16;
    return g;
}
constexpr Geometry geometry(int rows, int tile, int k) {
    if (k < 1 || k > kMaxK || (rows != 0 && !rows_ok(rows)) || (tile != 0 && !tile_ok(tile))) return Geometry{};
    const int t = tile ? tile : kDefaultTile;
    int r = rows ? rows : kDefaultRows;
    // the library's choice of rows: the most, up to kDefaultRows, whose lists fit
    while (!rows && r > 1 && (r * t > kNT * kPer || layout(r, t, k).lds > kLdsMax)) r /= 2;
    Geometry g = layout(r, t, k);
    if (r * t > kNT * kPer || g.lds > kLdsMax) g.lds = 0;
    return g;
}

struct SelectArgs {
    const void* Q;   // [d][n] queries
    const void* R;   // [d][m] candidates
    int f64;
    int metric;
    long long d, n, m;
    int k;
    long long width;  // candidates with |i - j| < width are left out; 0: none
    int skip_zero;    // candidates at distance exactly 0 are left out
    int* cnt;         // [n]
    int* idx;         // [n][k]
    double* dist;     // [n][k]
    Geometry g;
};

struct SortArgs {
    long long n;
    int k;
    const int* cnt;
    int* idx;
    double* dist;
};

struct MutualArgs {
    long long n;
    int k;
    const int* cnt;
    const int* idx;
    const double* dist;
    int sym, drop_zero;
    uint8_t* keep;  // [n][k]
};

struct BandwidthArgs {
    long long n;
    int k;
    const int* cnt;
    const double* dist;
    const uint8_t* keep;  // null: every entry is kept
    int add_self;         // the self link is stored, at distance 0
    int bandwidth_k;
    double* dist_to_k;    // [n]
    double* avg;          // [n]
    int* status;          // the status word, then the lowest empty row
};

struct MedianArgs {
    const double* v;  // [n]
    long long n;
    double* out;
    int* status;
};

struct CheckArgs {
    const double* v;
    long long count;
    int* status;
};

// what an entry is worth
struct Value {
    int mode, bw_mode;
    double bw_scalar;
    const double* bw_ptr;   // where the scalar bandwidth lies on the device (knn_median's), null: bw_scalar
    const double* sigma;    // [n] dist_to_k or avg, as the mode asks
    const double* matrix;   // [n][m]
    long long m;
};

struct EmitArgs {
    long long n, m;
    int k;
    const int* cnt;
    const int* idx;
    const double* dist;
    const uint8_t* keep;
    int self;          // the link (i, i) is stored
    Value val;
    int* counts;       // [n] (knn_count)
    int* indptr;       // [n + 1] (knn_scan); null with dense
    int* indices;      // [indptr[n]]
    void* data;        // uint8 (connectivity) or float64
    void* dense;       // [m][n], zero-filled; null with the sparse arrays
    long long* total;  // the entry count
};

struct DenseArgs {
    const void* Q;
    const void* R;
    int f64, metric;
    long long d, n, m;
    long long width;   // 0: every j is a candidate
    int self;
    Value val;
    void* out;         // [m][n] uint8 (connectivity) or float64
};

#ifdef LRA_POSTSIM
void knn_block_sync();
void knn_wave_sync();
unsigned long long knn_ballot(int pred);
void knn_status_or(int* word, int bits);
void knn_status_min(int* word, int v);
void knn_lds_add(int* word, int v);
#else
__device__ __forceinline__ void knn_block_sync() { __syncthreads(); }
// the LDS stores of the wave's lanes before this point are seen by its loads after it
__device__ __forceinline__ void knn_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ unsigned long long knn_ballot(int pred) { return __ballot(pred); }
__device__ __forceinline__ void knn_status_or(int* word, int bits) { atomicOr(word, bits); }
__device__ __forceinline__ void knn_status_min(int* word, int v) { atomicMin(word, v); }
__device__ __forceinline__ void knn_lds_add(int* word, int v) { atomicAdd(word, v); }
#endif

__device__ __forceinline__ double knn_nan() { return __builtin_nan(""); }

// the order of (distance, index) pairs: a NaN is larger than every number, an exact tie goes to the lower index
__device__ __forceinline__ bool knn_less(double d1, int i1, double d2, int i2) {
    const bool n1 = d1 != d1, n2 = d2 != d2;
    if (n1 || n2) return n1 == n2 ? i1 < i2 : n2;
    return d1 < d2 || (d1 == d2 && i1 < i2);
}

#ifdef LRA_POSTSIM
void knn_wave_max(double* d, int* i, int* p);
#else
// the largest of the lanes' (distance, index) pairs with its slot p (p < 0: the lane has none), left in every lane: a butterfly of six exchanges
__device__ __forceinline__ void knn_wave_max(double* d, int* i, int* p) {
#pragma unroll
    for (int s = kWave / 2; s > 0; s >>= 1) {
        const double od = __shfl_xor(*d, s, kWave);
        const int oi = __shfl_xor(*i, s, kWave), op = __shfl_xor(*p, s, kWave);
        if (op >= 0 && (*p < 0 || knn_less(*d, *i, od, oi))) { *d = od; *i = oi; *p = op; }
    }
}
#endif

// the largest pair of list[0 .. cnt) and its slot, the same in every lane of the wave
__device__ __forceinline__ void knn_list_max(const double* ld, const int* li, int cnt, int lane, double* td, int* ti, int* tp) {
    double bd = 0.0;
    int bi = -1, bp = -1;
    for (int e = lane; e < cnt; e += kWave)
        if (bp < 0 || knn_less(bd, bi, ld[e], li[e])) { bd = ld[e]; bi = li[e]; bp = e; }
    knn_wave_max(&bd, &bi, &bp);
    *td = bd;
    *ti = bi;
    *tp = bp;
}

// grid = ceil(n / g.rows) workgroups of kNT threads; dynamic LDS = g.lds.  METRIC: a.metric, known when the kernel is compiled (the sums of a
// thread's pairs then stay in registers)
template <int METRIC>
__device__ __forceinline__ void select_body(const SelectArgs& a) {
    LRA_KNN_DYN_LDS(lds);
    const Geometry& g = a.g;
    const int R = g.rows, T = g.tile, K = g.k, tid = (int)threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    double* xs = reinterpret_cast<double*>(lds);
    double* ys = reinterpret_cast<double*>(lds + g.off_y);
    double* dt = reinterpret_cast<double*>(lds + g.off_t);
    double* ld = reinterpret_cast<double*>(lds + g.off_ld);
    int* li = reinterpret_cast<int*>(lds + g.off_li);
    const long long i0 = (long long)blockIdx.x * R;
    const int rows = a.n - i0 < R ? (int)(a.n - i0) : R;
    const int pairs = R * T;
    // a wave's rows: r = wave + kWaves * q; their counts and thresholds in registers, the same in every lane
    constexpr int kOwn = kMaxRows / kWaves;
    int cnt[kOwn], thr_i[kOwn], thr_p[kOwn];
    double thr_d[kOwn];
#pragma unroll
    for (int q = 0; q < kOwn; ++q) { cnt[q] = 0; thr_i[q] = -1; thr_p[q] = -1; thr_d[q] = 0.0; }
    // the thread's distances of a tile: pair tid + p kNT is (row, column) = (pair / tile, pair % tile)
    int pr[kPer], pc[kPer];
#pragma unroll
    for (int p = 0; p < kPer; ++p) {
        pr[p] = (tid + p * kNT) / T;
        pc[p] = (tid + p * kNT) % T;
    }
    for (long long j0 = 0; j0 < a.m; j0 += T) {
        const int cols = a.m - j0 < T ? (int)(a.m - j0) : T;
        double acc[kPer], xx[kPer], yy[kPer];
#pragma unroll
        for (int p = 0; p < kPer; ++p) acc[p] = xx[p] = yy[p] = 0.0;
        for (long long f0 = 0; f0 < a.d; f0 += kFeat) {
            const int ff = a.d - f0 < kFeat ? (int)(a.d - f0) : kFeat;
            for (int q = tid; q < ff * R; q += kNT) {
                const int f = q / R, r = q % R;
                xs[f * R + r] = r < rows ? dtw::dtw_feature(a.Q, a.f64, (f0 + f) * a.n + i0 + r) : 0.0;
            }
            for (int q = tid; q < ff * T; q += kNT) {
                const int f = q / T, c = q % T;
                ys[f * T + c] = c < cols ? dtw::dtw_feature(a.R, a.f64, (f0 + f) * a.m + j0 + c) : 0.0;
            }
            knn_block_sync();
            for (int f = 0; f < ff; ++f) {
#pragma unroll
                for (int p = 0; p < kPer; ++p) {
                    const int at = tid + p * kNT;
                    if (at < pairs) dtw::dtw_metric_add(METRIC, xs[f * R + pr[p]], ys[f * T + pc[p]], acc[p], xx[p], yy[p]);
                }
            }
            knn_block_sync();
        }
#pragma unroll
        for (int p = 0; p < kPer; ++p) {
            const int at = tid + p * kNT;
            if (at < pairs) dt[at] = dtw::dtw_metric_finish(METRIC, acc[p], xx[p], yy[p]);
        }
        knn_block_sync();
#pragma unroll
        for (int q = 0; q < kOwn; ++q) {
            const int r = wave + kWaves * q;
            if (r < rows) {   // (the same for every lane of the wave)
                const long long i = i0 + r;
                double* rd = ld + (long long)r * K;
                int* ri = li + (long long)r * K;
                for (int c0 = 0; c0 < cols; c0 += kWave) {
                    const int c = c0 + lane;
                    const long long j = j0 + c;
                    const double dv = c < cols ? dt[r * T + c] : 0.0;
                    const long long gap = i > j ? i - j : j - i;
                    const bool cand = c < cols && !(gap < a.width) && !(a.skip_zero && dv == 0.0);
                    unsigned long long votes = knn_ballot(cand && (cnt[q] < K || knn_less(dv, (int)j, thr_d[q], thr_i[q])));
                    while (votes) {
                        const int b = __builtin_ctzll(votes);
                        votes &= votes - 1;
                        const double bd = dt[r * T + c0 + b];   // (every lane reads the same word)
                        const int bj = (int)(j0 + c0 + b);
                        if (cnt[q] < K) {
                            if (lane == 0) { rd[cnt[q]] = bd; ri[cnt[q]] = bj; }
                            ++cnt[q];
                            if (cnt[q] == K) {
                                knn_wave_sync();
                                knn_list_max(rd, ri, K, lane, &thr_d[q], &thr_i[q], &thr_p[q]);
                            }
                        } else if (knn_less(bd, bj, thr_d[q], thr_i[q])) {
                            if (lane == 0) { rd[thr_p[q]] = bd; ri[thr_p[q]] = bj; }
                            knn_wave_sync();
                            knn_list_max(rd, ri, K, lane, &thr_d[q], &thr_i[q], &thr_p[q]);
                            knn_wave_sync();   // (the list is read before the next winner is stored)
                        }
                    }
                }
            }
        }
        knn_block_sync();
    }
#pragma unroll
    for (int q = 0; q < kOwn; ++q) {
        const int r = wave + kWaves * q;
        if (r < rows) {
            const long long i = i0 + r;
            if (lane == 0) a.cnt[i] = cnt[q];
            for (int e = lane; e < cnt[q]; e += kWave) {
                a.idx[i * K + e] = li[(long long)r * K + e];
                a.dist[i * K + e] = ld[(long long)r * K + e];
            }
        }
    }
}

// grid = n workgroups of kSortNT threads; dynamic LDS = 12 k bytes
__device__ __forceinline__ void sort_rows_body(const SortArgs& a) {
    LRA_KNN_DYN_LDS(lds);
    double* sd = reinterpret_cast<double*>(lds);
    int* si = reinterpret_cast<int*>(lds + 8 * (long long)a.k);
    const long long i = blockIdx.x;
    const int c = a.cnt[i], tid = (int)threadIdx.x;
    for (int e = tid; e < c; e += kSortNT) {
        sd[e] = a.dist[i * a.k + e];
        si[e] = a.idx[i * a.k + e];
    }
    knn_block_sync();
    for (int e = tid; e < c; e += kSortNT) {
        const int mine = si[e];
        int rank = 0;
        for (int o = 0; o < c; ++o) rank += si[o] < mine;
        a.idx[i * a.k + rank] = mine;
        a.dist[i * a.k + rank] = sd[e];
    }
}

// grid = ceil(n k / kRowNT) workgroups of kRowNT threads
__device__ __forceinline__ void mutual_body(const MutualArgs& a) {
    const long long at = (long long)blockIdx.x * kRowNT + (long long)threadIdx.x;
    if (at >= a.n * a.k) return;
    const long long i = at / a.k;
    const int e = (int)(at % a.k);
    if (e >= a.cnt[i]) return;
    bool keep = !(a.drop_zero && a.dist[at] == 0.0);
    if (keep && a.sym) {
        const long long j = a.idx[at];
        const int* row = a.idx + j * a.k;
        int lo = 0, hi = j < a.n ? a.cnt[j] : 0;
        while (lo < hi) {
            const int mid = (lo + hi) / 2;
            if (row[mid] < i) lo = mid + 1; else hi = mid;
        }
        keep = j < a.n && lo < a.cnt[j] && row[lo] == i;
    }
    a.keep[at] = keep ? 1 : 0;
}

// grid = n workgroups of kRowNT threads; dynamic LDS = 16 (k + 1) bytes
__device__ __forceinline__ void bandwidth_body(const BandwidthArgs& a) {
    LRA_KNN_DYN_LDS(lds);
    double* raw = reinterpret_cast<double*>(lds);
    double* sorted = raw + (a.k + 1);
    __shared__ int kept;
    const long long i = blockIdx.x;
    const int c = a.cnt[i], tid = (int)threadIdx.x;
    // the kept distances in entry order, behind the self link's 0 (one thread: the rows are short and the order must not depend on timing)
    if (tid == 0) {
        int w = 0;
        if (a.add_self) raw[w++] = 0.0;
        for (int e = 0; e < c; ++e)
            if (!a.keep || a.keep[i * a.k + e]) raw[w++] = a.dist[i * a.k + e];
        kept = w;
    }
    knn_block_sync();
    const int w = kept;
    for (int e = tid; e < w; e += kRowNT) {
        const double mine = raw[e];
        int rank = 0;
        for (int o = 0; o < w; ++o) rank += knn_less(raw[o], o, mine, e);
        sorted[rank] = mine;
    }
    knn_block_sync();
    if (tid != 0) return;
    if (w == 0) {
        a.dist_to_k[i] = knn_nan();
        a.avg[i] = knn_nan();
        knn_status_or(a.status, kStatusRowEmpty);
        knn_status_min(a.status + 1, (int)i);
        return;
    }
    const int first = w < a.bandwidth_k ? w : a.bandwidth_k;
    double sum = 0.0;
    for (int e = 0; e < first; ++e) sum += sorted[e];
    a.dist_to_k[i] = sorted[first - 1];
    a.avg[i] = sum / (double)first;
}

// the integer key of a float64 whose unsigned order is the floats' order
__device__ __forceinline__ unsigned long long knn_key(double v) {
    const unsigned long long b = (unsigned long long)__builtin_bit_cast(long long, v);
    return b >> 63 ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double knn_unkey(unsigned long long key) {
    const unsigned long long b = key >> 63 ? key & 0x7fffffffffffffffull : ~key;
    return __builtin_bit_cast(double, (long long)b);
}

// one workgroup of kMedNT threads
__device__ __forceinline__ void median_body(const MedianArgs& a) {
    __shared__ int hist[256];
    __shared__ long long s_rank;
    __shared__ unsigned long long s_prefix;
    __shared__ int s_finite;
    const int tid = (int)threadIdx.x;
    if (tid == 0) s_finite = 0;
    hist[tid] = 0;
    knn_block_sync();
    {
        int mine = 0, finite = 0;
        for (long long q = tid; q < a.n; q += kMedNT) {
            const double v = a.v[q];
            mine += v == v;
            finite |= v == v && !dtw::dtw_isinf(v);
        }
        knn_lds_add(&hist[0], mine);
        if (finite) s_finite = 1;
    }
    knn_block_sync();
    const long long count = hist[0];
    const int any_finite = s_finite;
    knn_block_sync();
    if (!any_finite) {
        if (tid == 0) {
            knn_status_or(a.status, kStatusEmptyGraph);
            *a.out = knn_nan();
        }
        return;
    }
    double picked[2] = {0.0, 0.0};
    const long long ranks[2] = {(count - 1) / 2, count / 2};
    for (int which = 0; which < 2; ++which) {
        if (which == 1 && ranks[1] == ranks[0]) {
            picked[1] = picked[0];
            break;
        }
        if (tid == 0) { s_prefix = 0; s_rank = ranks[which]; }
        for (int pass = 0; pass < 8; ++pass) {
            const int shift = 56 - 8 * pass;
            hist[tid] = 0;
            knn_block_sync();
            const unsigned long long prefix = s_prefix;
            for (long long q = tid; q < a.n; q += kMedNT) {
                const double v = a.v[q];
                if (v != v) continue;
                const unsigned long long key = knn_key(v);
                if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) knn_lds_add(&hist[(int)((key >> shift) & 255)], 1);
            }
            knn_block_sync();
            if (tid == 0) {
                long long rank = s_rank;
                int digit = 0;
                while (digit < 255 && rank >= hist[digit]) rank -= hist[digit++];
                s_rank = rank;
                s_prefix = prefix | ((unsigned long long)digit << shift);
            }
            knn_block_sync();
        }
        picked[which] = knn_unkey(s_prefix);
        knn_block_sync();
    }
    if (tid == 0) *a.out = ranks[0] == ranks[1] ? picked[0] : (picked[0] + picked[1]) / 2.0;
}

// grid = ceil(count / kRowNT) workgroups of kRowNT threads
__device__ __forceinline__ void bw_check_body(const CheckArgs& a) {
    const long long at = (long long)blockIdx.x * kRowNT + (long long)threadIdx.x;
    if (at < a.count && a.v[at] <= 0.0) knn_status_or(a.status, kStatusNonPositive);
}

// the bandwidth of the entry (i, j) at distance d (__affinity_bandwidth :1352, :1360, :1401, :1412-1435)
__device__ __forceinline__ double knn_entry_bandwidth(const Value& v, long long i, long long j, double d) {
    switch (v.bw_mode) {
        case kBwScalar: return v.bw_ptr ? *v.bw_ptr : v.bw_scalar;
        case kBwMeanK:
        case kBwMeanKAvg: return (v.sigma[i] + v.sigma[j]) / 2.0;
        case kBwGmeanK:
        case kBwGmeanKAvg: return sqrt(v.sigma[i] * v.sigma[j]);
        case kBwMeanKAvgPair: return (v.sigma[i] + v.sigma[j] + d) / 3.0;
        default: return v.matrix[i * v.m + j];
    }
}

// exp(d / (-1 * bandwidth)) (:348, :698)
__device__ __forceinline__ double knn_affinity(double d, double bandwidth) { return exp(d / -bandwidth); }

// what the stored entry (i, j) at distance d holds, but for connectivity (a 1)
__device__ __forceinline__ double knn_value(const Value& v, long long i, long long j, double d) {
    return v.mode == kAffinity ? knn_affinity(d, knn_entry_bandwidth(v, i, j, d)) : d;
}

// grid = ceil(n / kRowNT) workgroups of kRowNT threads
__device__ __forceinline__ void count_body(const EmitArgs& a) {
    const long long i = (long long)blockIdx.x * kRowNT + (long long)threadIdx.x;
    if (i >= a.n) return;
    int c = a.self && i < a.m ? 1 : 0;
    for (int e = 0; e < a.cnt[i]; ++e) c += a.keep[i * a.k + e] != 0;
    a.counts[i] = c;
}

// one workgroup of kRowNT threads: indptr[0] = 0, indptr[i + 1] = counts[0] + ... + counts[i]
__device__ __forceinline__ void scan_body(const EmitArgs& a) {
    __shared__ long long part[kRowNT];
    const int tid = (int)threadIdx.x;
    const long long per = (a.n + kRowNT - 1) / kRowNT, lo = tid * per < a.n ? tid * per : a.n, hi = lo + per < a.n ? lo + per : a.n;
    long long sum = 0;
    for (long long i = lo; i < hi; ++i) sum += a.counts[i];
    part[tid] = sum;
    knn_block_sync();
    long long base = 0;
    for (int t = 0; t < tid; ++t) base += part[t];
    if (tid == 0) a.indptr[0] = 0;
    for (long long i = lo; i < hi; ++i) {
        base += a.counts[i];
        a.indptr[i + 1] = (int)base;
    }
    if (tid == kRowNT - 1) *a.total = base;
}

// grid = ceil(n / kRowNT) workgroups of kRowNT threads: row i's entries in index order, the self link in its place
__device__ __forceinline__ void emit_body(const EmitArgs& a) {
    const long long i = (long long)blockIdx.x * kRowNT + (long long)threadIdx.x;
    if (i >= a.n) return;
    const bool conn = a.val.mode == kConnectivity;
    long long at = a.indptr ? a.indptr[i] : 0;
    bool self = a.self && i < a.m;
    const int c = a.cnt[i];
    for (int e = 0; e <= c; ++e) {
        const bool last = e == c;
        const long long j = last ? a.m : a.idx[i * a.k + e];
        for (int turn = 0; turn < 2; ++turn) {
            // first the self link where it comes before entry e, then entry e
            const bool own = turn == 0;
            if (own ? !(self && i < j) : (last || !a.keep[i * a.k + e])) continue;
            const long long col = own ? i : j;
            const double d = own ? 0.0 : a.dist[i * a.k + e];
            if (own) self = false;
            if (a.dense) {
                if (conn) reinterpret_cast<uint8_t*>(a.dense)[col * a.n + i] = 1;
                else reinterpret_cast<double*>(a.dense)[col * a.n + i] = knn_value(a.val, i, col, d);
            } else {
                a.indices[at] = (int)col;
                if (conn) reinterpret_cast<uint8_t*>(a.data)[at] = 1;
                else reinterpret_cast<double*>(a.data)[at] = knn_value(a.val, i, col, d);
                ++at;
            }
        }
    }
}

// grid = ceil(n / kDenseTile) * ceil(m / kDenseTile) workgroups of kDenseNT threads; thread (ty, tx) forms out[j0 + ty + 8 q][i0 + tx], q < 4
__device__ __forceinline__ void dense_body(const DenseArgs& a) {
    __shared__ double xs[kFeat][kDenseTile];
    __shared__ double ys[kFeat][kDenseTile];
    constexpr int kEach = kDenseTile * kDenseTile / kDenseNT, kStep = kDenseNT / kDenseTile;
    const long long tiles_n = (a.n + kDenseTile - 1) / kDenseTile;
    const long long i0 = ((long long)blockIdx.x % tiles_n) * kDenseTile, j0 = ((long long)blockIdx.x / tiles_n) * kDenseTile;
    const int tid = (int)threadIdx.x, tx = tid % kDenseTile, ty = tid / kDenseTile;
    double acc[kEach], xx[kEach], yy[kEach];
#pragma unroll
    for (int q = 0; q < kEach; ++q) acc[q] = xx[q] = yy[q] = 0.0;
    for (long long f0 = 0; f0 < a.d; f0 += kFeat) {
        const int ff = a.d - f0 < kFeat ? (int)(a.d - f0) : kFeat;
        for (int q = tid; q < ff * kDenseTile; q += kDenseNT) {
            const int f = q / kDenseTile, c = q % kDenseTile;
            xs[f][c] = i0 + c < a.n ? dtw::dtw_feature(a.Q, a.f64, (f0 + f) * a.n + i0 + c) : 0.0;
            ys[f][c] = j0 + c < a.m ? dtw::dtw_feature(a.R, a.f64, (f0 + f) * a.m + j0 + c) : 0.0;
        }
        knn_block_sync();
        for (int f = 0; f < ff; ++f) {
            const double x = xs[f][tx];
#pragma unroll
            for (int q = 0; q < kEach; ++q) dtw::dtw_metric_add(a.metric, x, ys[f][ty + kStep * q], acc[q], xx[q], yy[q]);
        }
        knn_block_sync();
    }
    const bool conn = a.val.mode == kConnectivity;
#pragma unroll
    for (int q = 0; q < kEach; ++q) {
        const long long i = i0 + tx, j = j0 + ty + kStep * q;
        if (i >= a.n || j >= a.m) continue;
        const long long gap = i > j ? i - j : j - i;
        const bool own = a.self && i == j, cand = !(gap < a.width);
        const double d = dtw::dtw_metric_finish(a.metric, acc[q], xx[q], yy[q]);
        if (conn) {
            reinterpret_cast<uint8_t*>(a.out)[j * a.n + i] = own || cand ? 1 : 0;
        } else {
            double v = 0.0;
            if (own) v = knn_value(a.val, i, j, 0.0);
            else if (cand && d != 0.0) v = knn_value(a.val, i, j, d);
            reinterpret_cast<double*>(a.out)[j * a.n + i] = v;
        }
    }
}

// (plain functions, not templates: defined where LRA_KNN_KERNELS says so -- lra_knn_inst.hip and the simulator -- and nowhere else)
#if defined(LRA_KNN_KERNELS) || defined(LRA_POSTSIM)
__global__ __launch_bounds__(kNT) void knn_select_euclidean(SelectArgs a) { select_body<dtw::kEuclidean>(a); }
__global__ __launch_bounds__(kNT) void knn_select_sqeuclidean(SelectArgs a) { select_body<dtw::kSqeuclidean>(a); }
__global__ __launch_bounds__(kNT) void knn_select_cityblock(SelectArgs a) { select_body<dtw::kCityblock>(a); }
__global__ __launch_bounds__(kNT) void knn_select_cosine(SelectArgs a) { select_body<dtw::kCosine>(a); }
typedef void (*SelectKernel)(SelectArgs);
inline SelectKernel select_kernel(int metric) {
    static const SelectKernel table[4] = {knn_select_euclidean, knn_select_sqeuclidean, knn_select_cityblock, knn_select_cosine};
    return metric >= 0 && metric < 4 ? table[metric] : nullptr;
}
__global__ __launch_bounds__(kSortNT) void knn_sort_rows(SortArgs a) { sort_rows_body(a); }
__global__ __launch_bounds__(kRowNT) void knn_mutual(MutualArgs a) { mutual_body(a); }
__global__ __launch_bounds__(kRowNT) void knn_bandwidth(BandwidthArgs a) { bandwidth_body(a); }
__global__ __launch_bounds__(kMedNT) void knn_median(MedianArgs a) { median_body(a); }
__global__ __launch_bounds__(kRowNT) void knn_bw_check(CheckArgs a) { bw_check_body(a); }
__global__ __launch_bounds__(kRowNT) void knn_count(EmitArgs a) { count_body(a); }
__global__ __launch_bounds__(kRowNT) void knn_scan(EmitArgs a) { scan_body(a); }
__global__ __launch_bounds__(kRowNT) void knn_emit(EmitArgs a) { emit_body(a); }
__global__ __launch_bounds__(kDenseNT) void knn_dense(DenseArgs a) { dense_body(a); }
#endif

}  // namespace knn
}  // namespace lra
