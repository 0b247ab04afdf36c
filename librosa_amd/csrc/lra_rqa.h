// lra_rqa.h -- librosa.sequence.rqa (librosa/sequence.py:698-1074): the alignment score matrix, its pointers and the best alignment path, all
// on the device.
// Self-contained so that tests/hostsim/rqasim.cpp can run the same kernel bodies on host fibres (-DLRA_POSTSIM).
//
//   Row 0 and column 0: score = sim, pointer -2 where sim is non-zero (a NaN or a negative value counts) and -1 otherwise.  Cell (i, j), i, j >= 1,
//   takes its candidates in the order diagonal (i-1, j-1); with knight moves the left knight (i-1, j-2) if j >= 2 and the up knight (i-2, j-1) if
//   i >= 2.  s_c: the candidate's score as it was STORED (in sim's type), widened to float64; t_c = sim[candidate] > 0.
//       sim[i][j] > 0:  k = argmax(s);  score = s_k + sim[i][j] (one float64 sum, rounded once to sim's type by the store);  pointer = k
//       otherwise:      v_c = (s_c - t_c * gap_onset) - (!t_c) * gap_extend, every operation rounded on its own (0 * inf is NaN: an infinite gap makes
//                       every v_c NaN);  k = argmax(v);  score = v_k > 0 ? v_k : +0.0;  pointer = k where the stored score is non-zero, else -1
//   argmax is NumPy's: the first maximum, a NaN counts as the maximum and the first NaN wins.  hipcc would contract s - t * gap into a fused
//   multiply-add, which rounds once and gives other bits than the reference, so the function that forms candidates carries
//   `#pragma clang fp contract(off)`.  The pointers are the device's own codes: 0 diagonal, 1 left knight (-1, -2), 2 up knight (-2, -1) -- the move
//   that was scored, also in column 1 where the reference numbers the up knight 1.
//
//   rqa_score      The recurrence has no dependency inside a row: cell (i, j) reads rows i-1 and i-2 at columns j-1 and j-2 only.  The matrix is cut
//                  into blocks of R rows, one launch per block in stream order, and into strips of W columns, one workgroup per strip; no workgroup
//                  ever waits for another.  A workgroup sweeps its block's rows top to bottom and sees of other strips only the finished rows above
//                  the block: it recomputes the left halo itself, row r of a block of nb rows starting at column max(0, c0 - 2 (nb - 1 - r)).  The
//                  last two rows rotate through three row buffers in LDS, one barrier per row that waits for the LDS alone (nothing in a launch
//                  reads back what it stored to memory).  A cell keeps there its stored score as float64 and, formed once, what it is worth to a
//                  successor without a hit, (s - t * gap_onset) - (!t) * gap_extend: that value depends on the candidate alone.  sim is fetched a
//                  chunk of kChunk rows ahead of the chunk being swept.  Only the strip's own columns are stored: score in sim's type, the
//                  pointers as int8.
//   rqa_argmax     np.argmax(score) in two stages: a NaN first, otherwise the maximum with the lowest flat index.
//   rqa_backtrack  one thread walks the pointers from that cell, prepending cells: it stops before a -1 cell and after a -2 cell.  Every move lowers
//                  both indices, so a path holds at most min(N, M) cells; it is filled from the back of a [min(N, M)][2] uint64 buffer.
// Everything that scales with N * M is indexed in 64 bits.
#pragma once

#ifndef LRA_POSTSIM
#include <hip/hip_runtime.h>
#endif

#include <cstdint>

#ifdef LRA_POSTSIM
#define LRA_RQA_DYN_LDS(ptr) char* ptr = reinterpret_cast<char*>(g_postsim_dyn_lds)
#else
#define LRA_RQA_DYN_LDS(ptr) extern __shared__ __align__(16) char lra_rqa_lds[]; char* ptr = lra_rqa_lds
#endif

namespace lra {
namespace rqa {

constexpr int kDefaultRows = 64;     // rows of a block (a launch)
constexpr int kDefaultStrip = 64;    // columns of a strip (a workgroup)
constexpr int kF32 = 0, kF64 = 1;    // LRA_F32, LRA_F64: the types of sim and score
constexpr int kScoreNT = 256;        // the most threads of a scoring workgroup (a narrow strip takes fewer: Geometry::nt)
constexpr int kChunk = 6;            // rows of sim fetched together, one chunk ahead of the sweep; a multiple of 3: a chunk starts on LDS row buffer 2
constexpr int kMaxIters = 5;         // cells of a row per thread: ceil((1024 + 2 * 63) / 256)
constexpr int kArgNT = 256;
constexpr int kArgPer = 16;          // elements per thread and pass of the first stage
constexpr int kMaxParts = 1024;      // partial results of the first stage
constexpr int kWorkBytes = 16 + 16 * kMaxParts;   // LRA_RQA_WORK_BYTES: the flat index, the length, the partial indices, the partial values

constexpr bool rows_ok(int rows) { return rows == 1 || rows == 2 || rows == 4 || rows == 8 || rows == 16 || rows == 32 || rows == 64; }
constexpr bool strip_ok(int strip) { return strip >= 4 && strip <= 1024 && (strip & (strip - 1)) == 0; }

// what a scoring launch looks like for (rows, strip), 0: the library's choice
struct Geometry {
    int rows, strip;
    int halo;      // columns recomputed to the left of the strip in the block's first row: 2 (rows - 1)
    int width;     // columns of an LDS row: strip + halo + 2 (the two columns the first computed cell looks back to)
    int nt;        // threads of a workgroup: strip + halo rounded up to whole waves, kScoreNT at the most
    int iters;     // cells of a row per thread
    int lds;       // bytes of dynamic LDS: three rows of (score, gap value) pairs
};
constexpr Geometry geometry(int rows, int strip) {
    Geometry g{};
    g.rows = rows ? rows : kDefaultRows;
    g.strip = strip ? strip : kDefaultStrip;
    g.halo = 2 * (g.rows - 1);
    g.width = g.strip + g.halo + 2;
    g.nt = (g.strip + g.halo + 63) / 64 * 64 < kScoreNT ? (g.strip + g.halo + 63) / 64 * 64 : kScoreNT;
    g.iters = (g.strip + g.halo + g.nt - 1) / g.nt;
    g.lds = 3 * g.width * 16;
    return g;
}

struct ScoreArgs {
    const void* sim;  // [N][M] float32 or float64, never written
    int f64;
    long long N, M;
    double gap_onset, gap_extend;
    int knight;
    void* score;      // [N][M] of sim's type
    int8_t* ptr;      // [N][M]
    long long row0;   // the block's first row
    Geometry g;
};

struct ArgmaxArgs {
    const void* score;
    int f64;
    long long count;
    int parts;
    long long* part_i;  // [parts]
    double* part_v;     // [parts]
    long long* out;     // the flat index
};

struct BackArgs {
    const int8_t* ptr;  // [N][M]
    long long N, M;
    const long long* start;  // the flat index of the last cell
    unsigned long long* path;  // [cap][2], filled from the back
    long long cap;
    long long* length;
};

__device__ __forceinline__ double rqa_load(const void* p, int f64, long long at) {
    return f64 ? reinterpret_cast<const double*>(p)[at] : (double)reinterpret_cast<const float*>(p)[at];
}

// np.argmax's order over candidates taken in turn: c replaces best where best is no NaN and c is a NaN or greater
__device__ __forceinline__ bool rqa_takes(double c, double best) { return !(best != best) && (c != c || c > best); }

// np.argmax's order over (value, flat index) pairs in any order; an index < 0: nothing there
__device__ __forceinline__ bool rqa_argmax_better(double v, long long i, double bv, long long bi) {
    if (i < 0) return false;
    if (bi < 0) return true;
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

#ifdef LRA_POSTSIM
void rqa_lds_sync();
#else
// the LDS stores of the workgroup before this point are seen by its LDS loads after it; stores to global memory are not waited for
__device__ __forceinline__ void rqa_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
#endif

// t * gap_onset and (!t) * gap_extend for both values of t, each one product as the reference forms it (0 * inf is NaN)
struct Gaps {
    double onset_t, onset_f, extend_t, extend_f;
};
__device__ __forceinline__ Gaps rqa_gaps(double gap_onset, double gap_extend) {
#pragma clang fp contract(off)
    Gaps g;
    g.onset_t = 1.0 * gap_onset;
    g.onset_f = 0.0 * gap_onset;
    g.extend_t = 0.0 * gap_extend;
    g.extend_f = 1.0 * gap_extend;
    return g;
}

// what a finished cell (its stored score s, t = sim > 0 there) is worth as a candidate of a cell without a hit: (s - t * gap_onset) - (!t) * gap_extend.
// It depends on the candidate alone, so the cell that owns it forms it once and its three successors read it
__device__ __forceinline__ double rqa_gap_value(double s, bool t, const Gaps& g) {
#pragma clang fp contract(off)
    double v = s - (t ? g.onset_t : g.onset_f);
    v = v - (t ? g.extend_t : g.extend_f);
    return v;
}

// a finished cell in LDS: the stored score (widened), and rqa_gap_value of it
struct alignas(16) Pair {
    double s, g;
};

// one cell i, j >= 1: sv = sim[i][j]; c0, c1, c2 the candidates' values (their scores where sv > 0, else their gap values), has1 / has2: the knights
// exist.  Returns the score as it is stored (rounded to sim's type, widened again); *code: the pointer
template <typename T>
__device__ __forceinline__ double rqa_cell(double sv, double c0, double c1, bool has1, double c2, bool has2, int* code) {
#pragma clang fp contract(off)
    const bool hit = sv > 0.0;
    double best = c0;
    int k = 0;
    if (has1 && rqa_takes(c1, best)) { best = c1; k = 1; }
    if (has2 && rqa_takes(c2, best)) { best = c2; k = 2; }
    double out = hit ? best + sv : (best > 0.0 ? best : 0.0);
    out = (double)(T)out;
    *code = hit || out != 0.0 ? k : -1;
    return out;
}

// Local column l of a workgroup is global column base + l, base = c0 - halo - 2; what bounds a row in local columns:
struct Columns {
    int first;   // the first column inside the matrix: max(0, -base)
    int end;     // c1 - base
    int col0;    // global column 0, or -1 where the strip does not reach it
    int from2;   // global column 2 (the left knight exists from here on), 0 where it lies to the left of the LDS row
};

// the chunk of sim rows r0 .. r0 + kChunk - 1 of the block, the cells this thread computes (0 elsewhere)
template <int IT, typename T>
__device__ __forceinline__ void score_fetch(const ScoreArgs& a, int r0, int nb, const Columns& c, long long base, int tid, T (&v)[kChunk][IT]) {
    const T* sim = reinterpret_cast<const T*>(a.sim);
#pragma unroll
    for (int q = 0; q < kChunk; ++q) {
        const int r = r0 + q, start = a.g.halo + 2 - 2 * (nb - 1 - r);
        const long long row_at = (a.row0 + r) * a.M + base;
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int l = 2 + tid + k * a.g.nt;
            const bool ok = r < nb && l >= c.first && l >= start && l < c.end;
            v[q][k] = ok ? sim[row_at + l] : (T)0;
        }
    }
}

// grid = ceil(M / strip) workgroups of g.nt threads; dynamic LDS = g.lds.  IT = g.iters.  Block-relative row r lives in LDS row buffer
// (r + 2) % 3.  T: the type of sim and score
template <int IT, typename T>
__device__ __forceinline__ void score_body(const ScoreArgs& a) {
    LRA_RQA_DYN_LDS(lds);
    const Geometry& g = a.g;
    const int width = g.width, nt = g.nt, tid = (int)threadIdx.x;
    Pair* S = reinterpret_cast<Pair*>(lds);
    const long long N = a.N, M = a.M, i0 = a.row0;
    const long long c0 = (long long)blockIdx.x * g.strip, c1 = M - c0 < g.strip ? M : c0 + g.strip;
    const int nb = N - i0 < g.rows ? (int)(N - i0) : g.rows;
    const long long base = c0 - g.halo - 2;
    Columns c;
    c.first = base < 0 ? (int)-base : 0;
    c.end = (int)(c1 - base);
    c.col0 = base <= 0 ? (int)-base : -1;
    c.from2 = base < 2 ? (int)(2 - base) : 0;
    const int own = g.halo + 2;   // the strip's own columns start here
    const Gaps gaps = rqa_gaps(a.gap_onset, a.gap_extend);
    static_assert(kChunk % 3 == 0, "the row buffers of a chunk are known when it is compiled");
    const T* sim = reinterpret_cast<const T*>(a.sim);
    T* score = reinterpret_cast<T*>(a.score);
    T ahead[kChunk][IT];
    score_fetch<IT, T>(a, 0, nb, c, base, tid, ahead);
    // the two finished rows above the block (nothing is read of a row above the matrix)
    for (int q = 1; q <= 2; ++q) {
        const long long gi = i0 - q;
        Pair* row = S + ((2 - q) % 3) * width;
        for (int l = tid; l < width; l += nt) {
            const bool in = gi >= 0 && l >= c.first && l < c.end;
            const double sc = in ? (double)score[gi * M + base + l] : 0.0;
            const bool t = in && sim[gi * M + base + l] > (T)0;
            row[l] = Pair{sc, rqa_gap_value(sc, t, gaps)};
        }
    }
    rqa_lds_sync();
    for (int r0 = 0; r0 < nb; r0 += kChunk) {
        T sv[kChunk][IT];
#pragma unroll
        for (int q = 0; q < kChunk; ++q)
#pragma unroll
            for (int k = 0; k < IT; ++k) sv[q][k] = ahead[q][k];
        if (r0 + kChunk < nb) score_fetch<IT, T>(a, r0 + kChunk, nb, c, base, tid, ahead);   // (the same for every thread of the workgroup)
#pragma unroll
        for (int q = 0; q < kChunk; ++q) {
            const int r = r0 + q;
            if (r < nb) {   // (the same for every thread of the workgroup)
                const long long gi = i0 + r, row_at = gi * M + base;
                const int start = own - 2 * (nb - 1 - r);
                const bool has2 = a.knight && gi >= 2;
                Pair* cur = S + ((q + 2) % 3) * width;   // (r0 is a multiple of 3)
                const Pair* p1 = S + ((q + 1) % 3) * width;
                const Pair* p2 = S + (q % 3) * width;
#pragma unroll
                for (int k = 0; k < IT; ++k) {
                    const int l = 2 + tid + k * nt;
                    if (l >= c.first && l >= start && l < c.end) {
                        const double v = (double)sv[q][k];
                        const bool hit = v > 0.0;
                        double out;
                        int code;
                        if (gi == 0 || l == c.col0) {
                            out = v;
                            code = v != 0.0 ? -2 : -1;
                        } else {
                            const Pair d = p1[l - 1], kl = p1[l - 2], ku = p2[l - 1];
                            out = rqa_cell<T>(v, hit ? d.s : d.g, hit ? kl.s : kl.g, a.knight && l >= c.from2, hit ? ku.s : ku.g, has2, &code);
                        }
                        cur[l] = Pair{out, rqa_gap_value(out, hit, gaps)};
                        if (l >= own) {
                            score[row_at + l] = (T)out;
                            a.ptr[row_at + l] = (int8_t)code;
                        }
                    }
                }
            }
            rqa_lds_sync();
        }
    }
}

// grid = parts workgroups of kArgNT threads: workgroup b reduces the elements b kArgNT kArgPer + [0, kArgNT kArgPer), + parts kArgNT kArgPer, ...
__device__ __forceinline__ void argmax_reduce(double* red_v, long long* red_i, double bv, long long bi, int tid) {
    red_v[tid] = bv;
    red_i[tid] = bi;
    __syncthreads();
    for (int s = kArgNT / 2; s > 0; s >>= 1) {
        if (tid < s && rqa_argmax_better(red_v[tid + s], red_i[tid + s], red_v[tid], red_i[tid])) {
            red_v[tid] = red_v[tid + s];
            red_i[tid] = red_i[tid + s];
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void argmax_part_body(const ArgmaxArgs& a) {
    __shared__ double red_v[kArgNT];
    __shared__ long long red_i[kArgNT];
    const int tid = (int)threadIdx.x;
    const long long span = (long long)kArgNT * kArgPer;
    double bv = 0.0;
    long long bi = -1;
    for (long long at0 = (long long)blockIdx.x * span; at0 < a.count; at0 += (long long)a.parts * span) {
#pragma unroll
        for (int k = 0; k < kArgPer; ++k) {
            const long long at = at0 + (long long)k * kArgNT + tid;
            if (at < a.count) {
                const double v = rqa_load(a.score, a.f64, at);
                if (rqa_argmax_better(v, at, bv, bi)) { bv = v; bi = at; }
            }
        }
    }
    argmax_reduce(red_v, red_i, bv, bi, tid);
    if (tid == 0) {
        a.part_v[blockIdx.x] = red_v[0];
        a.part_i[blockIdx.x] = red_i[0];
    }
}

// one workgroup of kArgNT threads
__device__ __forceinline__ void argmax_final_body(const ArgmaxArgs& a) {
    __shared__ double red_v[kArgNT];
    __shared__ long long red_i[kArgNT];
    const int tid = (int)threadIdx.x;
    double bv = 0.0;
    long long bi = -1;
    for (int p = tid; p < a.parts; p += kArgNT)
        if (rqa_argmax_better(a.part_v[p], a.part_i[p], bv, bi)) { bv = a.part_v[p]; bi = a.part_i[p]; }
    argmax_reduce(red_v, red_i, bv, bi, tid);
    if (tid == 0) *a.out = red_i[0];
}

// one thread
__device__ __forceinline__ void backtrack_body(const BackArgs& a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    long long i = *a.start / a.M, j = *a.start % a.M, len = 0;
    while (i >= 0 && j >= 0 && len < a.cap) {
        const int code = (int)a.ptr[i * a.M + j];
        if (code == -1) break;   // a reset that is not part of the path
        ++len;
        a.path[2 * (a.cap - len)] = (unsigned long long)i;
        a.path[2 * (a.cap - len) + 1] = (unsigned long long)j;
        if (code == -2) break;   // the start of the sequence
        i -= code == 2 ? 2 : 1;
        j -= code == 1 ? 2 : 1;
    }
    *a.length = len;
}

// (plain functions, not templates: defined where LRA_RQA_KERNELS says so -- lra_rqa_inst.hip and the simulator -- and nowhere else)
#if defined(LRA_RQA_KERNELS) || defined(LRA_POSTSIM)
__global__ __launch_bounds__(kScoreNT) void rqa_score_f32_1(ScoreArgs a) { score_body<1, float>(a); }
__global__ __launch_bounds__(kScoreNT) void rqa_score_f32_2(ScoreArgs a) { score_body<2, float>(a); }
__global__ __launch_bounds__(kScoreNT) void rqa_score_f32_3(ScoreArgs a) { score_body<3, float>(a); }
__global__ __launch_bounds__(kScoreNT) void rqa_score_f32_4(ScoreArgs a) { score_body<4, float>(a); }
__global__ __launch_bounds__(kScoreNT) void rqa_score_f32_5(ScoreArgs a) { score_body<5, float>(a); }
__global__ __launch_bounds__(kScoreNT) void rqa_score_f64_1(ScoreArgs a) { score_body<1, double>(a); }
__global__ __launch_bounds__(kScoreNT) void rqa_score_f64_2(ScoreArgs a) { score_body<2, double>(a); }
__global__ __launch_bounds__(kScoreNT) void rqa_score_f64_3(ScoreArgs a) { score_body<3, double>(a); }
__global__ __launch_bounds__(kScoreNT) void rqa_score_f64_4(ScoreArgs a) { score_body<4, double>(a); }
__global__ __launch_bounds__(kScoreNT) void rqa_score_f64_5(ScoreArgs a) { score_body<5, double>(a); }
__global__ __launch_bounds__(kArgNT) void rqa_argmax_part(ArgmaxArgs a) { argmax_part_body(a); }
__global__ __launch_bounds__(kArgNT) void rqa_argmax_final(ArgmaxArgs a) { argmax_final_body(a); }
__global__ __launch_bounds__(64) void rqa_backtrack(BackArgs a) { backtrack_body(a); }
typedef void (*ScoreKernel)(ScoreArgs);
inline ScoreKernel score_kernel(int iters, int f64) {
    static const ScoreKernel table[2][kMaxIters] = {{rqa_score_f32_1, rqa_score_f32_2, rqa_score_f32_3, rqa_score_f32_4, rqa_score_f32_5},
                                                    {rqa_score_f64_1, rqa_score_f64_2, rqa_score_f64_3, rqa_score_f64_4, rqa_score_f64_5}};
    return iters >= 1 && iters <= kMaxIters ? table[f64 != 0][iters - 1] : nullptr;
}
#endif

// the workgroups of the first argmax stage
constexpr int argmax_parts(long long count) {
    const long long span = (long long)kArgNT * kArgPer, want = (count + span - 1) / span;
    return want < 1 ? 1 : (want > kMaxParts ? kMaxParts : (int)want);
}

}  // namespace rqa
}  // namespace lra
