// lra_viterbi.h -- librosa.sequence.viterbi, viterbi_discriminative and viterbi_binary (librosa/sequence.py:1174-1874): the log observation
// table prepared on the device, and the decode of every sequence of a batch in one launch.
// Self-contained so that tests/hostsim/viterbisim.cpp can run the same kernel bodies on host threads (-DLRA_POSTSIM).
//
//   value[0][j] = log_prob[0][j] + log_p_init[j]
//   value[t][j] = log_prob[t][j] + max_k (value[t - 1][k] + log_trans[k][j]),  ptr[t][j] = the first k that reaches the maximum (0 where every
//                                                                              candidate is -inf); with a threshold k runs over the
//                                                                              predecessors with log_trans[k][j] >= threshold only
//   state[T - 1] = np.argmax(value[T - 1]),  state[t] = ptr[t + 1][state[t + 1]],  logp = value[T - 1][state[T - 1]]
// Every operation is one correctly rounded float64 addition or a comparison, so the candidates of a target may be dealt over lanes and joined
// in any order as long as the join prefers the larger cost and, on equal cost, the lower k: the result is the reference's bit for bit.
//
//   viterbi_prep         prob [clip][state][step] (step contiguous) -> log_prob [clip][step][state] float64 through an LDS tile of kPrepStates x
//                        kPrepSteps: log(prob + eps) in prob's precision, minus log_marginal[state] (discriminative); kLog: the transpose alone.
//                        Range flags (negative, above one, column sum not close to one) are ORed into one word that the host reads before the decode.
//   viterbi_prep_binary  prob [chain][step] -> log_prob [chain][step][2]: the rows 1 - p and p of viterbi_binary formed here (elementwise).
//   viterbi_wg           one workgroup per sequence, n_states > kSmallMax.  The two live value rows are double-buffered in LDS, one barrier per step.
//                        A target's candidates are dealt over `lanes` lanes of one wave (a power of two; 1 once there are as many targets as
//                        threads) and joined by shuffles.  Full search reads log_trans[k][j] row by row (neighbouring lanes read neighbouring j),
//                        from LDS where the table fits beside the value rows, through L2 otherwise.  Thresholded search reads the predecessor
//                        lists in the target-minor layout [e][j].  ptr goes to a uint16 scratch [clip][step][state]; after the last step the
//                        workgroup reduces the argmax and one thread walks the pointers back.
//   viterbi_small        n_states <= kSmallMax: one chain per group of pow2ceil(n_states) lanes, many chains per workgroup, the value row in
//                        registers (lane j holds value[j], read by shuffles), the chain's own table in LDS (chain % n_tables: viterbi_binary's
//                        per-label (2, 2) tables).  The threshold is applied as a comparison, which visits the same candidates in the same order
//                        as the lists.
// The geometry depends on n_states and the list length alone, so a sequence gives the same bits alone and inside a batch.
#pragma once

#ifndef LRA_POSTSIM
#include <hip/hip_runtime.h>
#endif

#include <cstdint>

#ifdef LRA_POSTSIM
#define LRA_VIT_DYN_LDS(ptr) char* ptr = reinterpret_cast<char*>(g_postsim_dyn_lds)
#else
#define LRA_VIT_DYN_LDS(ptr) extern __shared__ __align__(16) char lra_vit_lds[]; char* ptr = lra_vit_lds
#endif

namespace lra {
namespace viterbi {

constexpr int kGenerative = 0, kDiscriminative = 1, kBinary = 2, kLog = 3;  // the LRA_VITERBI_* kinds of include/librosa_amd.h
constexpr int kFlagNegative = 1, kFlagAboveOne = 2, kFlagColumnSum = 4;     // the LRA_VITERBI_FLAG_* bits
constexpr int kSmallMax = 32;      // states of the small kernel
constexpr int kMaxStates = 8192;   // 16 bytes of value rows per state and the argmax scratch within kLdsMax
constexpr int kLdsMax = 160 * 1024;
constexpr int kPrepNT = 256, kPrepSteps = 32, kPrepStates = 64;
constexpr int kSmallNT = 256;
constexpr int kWgMaxNT = 1024;

constexpr int pow2_ceil(int n) {
    int p = 1;
    while (p < n) p *= 2;
    return p;
}

// what a decode launch looks like for n_states and, with a threshold, the longest predecessor list n_pred (0: full search)
struct Geometry {
    int small;      // the small kernel
    int nt;         // threads per workgroup
    int lanes;      // lanes per target (wg) or per chain (small)
    int table_lds;  // wg, full search: log_trans held in LDS
    int lds;        // bytes of dynamic LDS
};
constexpr Geometry geometry(int S, int n_pred) {
    Geometry g{};
    if (S <= kSmallMax) {
        g.small = 1;
        g.nt = kSmallNT;
        g.lanes = pow2_ceil(S);
        g.lds = (kSmallNT / g.lanes) * S * S * 8;
        return g;
    }
    const int cand = n_pred > 0 ? n_pred : S;
    if (S <= 128) {
        // fewer targets than the threads of four waves: the candidates of a target are dealt over lanes
        g.nt = 256;
        g.lanes = 256 / pow2_ceil(S);
        while (g.lanes > 1 && g.lanes > cand) g.lanes /= 2;
    } else {
        const int passes = (S + kWgMaxNT - 1) / kWgMaxNT;
        g.nt = ((S + passes - 1) / passes + 63) / 64 * 64;
        g.lanes = 1;
    }
    g.lds = 16 * S + 12 * g.nt;  // two value rows; the argmax scratch (a float64 and an int per thread)
    if (n_pred == 0 && (long long)g.lds + 8LL * S * S <= kLdsMax) {
        g.table_lds = 1;
        g.lds += 8 * S * S;
    }
    return g;
}

struct Args {
    const double* log_prob;    // [chain][step][state]
    const double* log_trans;   // [table][state][state]
    const double* log_p_init;  // [table][state]
    int n_tables;              // chain c reads table c % n_tables (1 in the wg kernel)
    long long chains;
    int S;
    long long T;
    double threshold;          // small kernel: candidates with log_trans >= threshold (-inf: all of them)
    int n_pred;                // wg kernel: rows of the predecessor lists (0: full search)
    const uint16_t* pred_k;    // [n_pred][state]
    const double* pred_lt;     // [n_pred][state]
    const int* pred_n;         // [state] length of the target's list
    uint16_t* ptr;             // scratch [chain][step][state]
    uint16_t* states;          // [chain][step]
    double* logp;              // [chain]
    Geometry g;
};

struct PrepArgs {
    const void* prob;            // [clip][state][step], or [chain][step] (binary)
    int f64;
    int kind;
    long long clips;             // binary: chains
    int S;                       // binary: 2
    long long T;
    double eps;                  // tiny of prob's type (binary: of float64)
    const double* log_marginal;  // discriminative: [state]; binary: [label][2]
    int n_labels;                // binary: chain c is label c % n_labels
    double* log_prob;
    int* flags;
};

#ifdef LRA_POSTSIM
double vit_shfl(double v, int lane);  // the value of lane `lane` of the same wave
double vit_shfl_xor(double v, int offset);
int vit_shfl_xor(int v, int offset);
void vit_flag_or(int* word, int bits);
#else
__device__ __forceinline__ double vit_shfl(double v, int lane) { return __shfl(v, lane, 64); }
__device__ __forceinline__ double vit_shfl_xor(double v, int offset) { return __shfl_xor(v, offset, 64); }
__device__ __forceinline__ int vit_shfl_xor(int v, int offset) { return __shfl_xor(v, offset, 64); }
__device__ __forceinline__ void vit_flag_or(int* word, int bits) { atomicOr(word, bits); }
#endif

__device__ __forceinline__ double vit_neg_inf() { return -__builtin_huge_val(); }

// np.argmax's order: the first NaN wins; otherwise the larger value, the lower index on a tie; an index < 0: nothing there
__device__ __forceinline__ bool vit_argmax_better(double v, int i, double bv, int bi) {
    if (i < 0) return false;
    if (bi < 0) return true;
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

// log(x + eps) in prob's precision, widened exactly (np.log(prob + tiny(prob)))
__device__ __forceinline__ double vit_log(const PrepArgs& a, double x) {
    if (a.f64) return log(x + a.eps);
    const float y = (float)x + (float)a.eps;
    return (double)logf(y);
}

__device__ __forceinline__ double vit_load(const PrepArgs& a, long long at) {
    return a.f64 ? reinterpret_cast<const double*>(a.prob)[at] : (double)reinterpret_cast<const float*>(a.prob)[at];
}

// grid = clips * ceil(T / kPrepSteps) workgroups of kPrepNT threads; a workgroup walks every state tile of its steps
__device__ __forceinline__ void prep_body(const PrepArgs& a) {
    __shared__ double tile[kPrepStates][kPrepSteps + 1];
    __shared__ double part[kPrepNT / kPrepSteps][kPrepSteps];
    const long long tiles = (a.T + kPrepSteps - 1) / kPrepSteps;
    const long long clip = (long long)blockIdx.x / tiles, t0 = ((long long)blockIdx.x % tiles) * kPrepSteps;
    const int tid = (int)threadIdx.x, tx = tid % kPrepSteps, ty = tid / kPrepSteps, S = a.S;
    constexpr int kRows = kPrepNT / kPrepSteps;
    double colsum = 0.0;
    int flags = 0;
    for (int s0 = 0; s0 < S; s0 += kPrepStates) {
        for (int r = ty; r < kPrepStates; r += kRows) {
            const int s = s0 + r;
            const long long t = t0 + tx;
            if (s < S && t < a.T) {
                const double x = vit_load(a, (clip * S + s) * a.T + t);
                if (a.kind == kLog) {
                    tile[r][tx] = x;
                } else {
                    if (x < 0.0) flags |= kFlagNegative;
                    if (x > 1.0) flags |= kFlagAboveOne;
                    colsum += x;
                    double v = vit_log(a, x);
                    if (a.kind == kDiscriminative) v -= a.log_marginal[s];
                    tile[r][tx] = v;
                }
            }
        }
        __syncthreads();
        for (int q = tid; q < kPrepStates * kPrepSteps; q += kPrepNT) {
            const int r = q % kPrepStates, c = q / kPrepStates;
            const int s = s0 + r;
            const long long t = t0 + c;
            if (s < S && t < a.T) a.log_prob[(clip * a.T + t) * S + s] = tile[r][c];
        }
        __syncthreads();
    }
    if (a.kind == kDiscriminative) {
        // np.allclose(prob.sum(axis=-2), 1): |sum - 1| <= 1e-8 + 1e-5, false for a NaN
        part[ty][tx] = colsum;
        __syncthreads();
        if (ty == 0 && t0 + tx < a.T) {
            double s = 0.0;
            for (int r = 0; r < kRows; ++r) s += part[r][tx];
            if (!(__builtin_fabs(s - 1.0) <= 1e-8 + 1e-5)) flags |= kFlagColumnSum;
        }
    }
    if (flags) vit_flag_or(a.flags, flags);
}

// grid = ceil(chains * T / kPrepNT) workgroups of kPrepNT threads
__device__ __forceinline__ void prep_binary_body(const PrepArgs& a) {
    const long long at = (long long)blockIdx.x * kPrepNT + (long long)threadIdx.x;
    if (at >= a.clips * a.T) return;
    const long long chain = at / a.T;
    const int label = (int)(chain % a.n_labels);
    const double p = vit_load(a, at);
    // 1 - prob in prob's precision, stored to a float64 row (sequence.py:1853-1854); the logarithm is float64's from there on
    const double q = a.f64 ? 1.0 - p : (double)(1.0f - (float)p);
    int flags = 0;
    if (p < 0.0) flags |= kFlagNegative;
    if (p > 1.0) flags |= kFlagAboveOne;
    a.log_prob[2 * at] = log(q + a.eps) - a.log_marginal[2 * label];
    a.log_prob[2 * at + 1] = log(p + a.eps) - a.log_marginal[2 * label + 1];
    if (flags) vit_flag_or(a.flags, flags);
}

// grid = chains workgroups of g.nt threads; dynamic LDS = g.lds
__device__ __forceinline__ void wg_body(const Args& a) {
    LRA_VIT_DYN_LDS(lds);
    const int S = a.S, nt = a.g.nt, G = a.g.lanes, W = 64 / G;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int slot = wave * W + (lane & (W - 1)), sub = lane / W;  // the lanes of a target are W apart: neighbouring lanes hold neighbouring targets
    const int per_pass = (nt >> 6) * W;
    double* prev = reinterpret_cast<double*>(lds);
    double* cur = prev + S;
    double* red_v = cur + S;
    int* red_i = reinterpret_cast<int*>(red_v + nt);
    double* tab = reinterpret_cast<double*>(red_i + nt);
    const long long chain = blockIdx.x;
    const double* lp = a.log_prob + chain * a.T * S;
    uint16_t* ptr = a.ptr + chain * a.T * S;
    if (a.g.table_lds)
        for (int i = tid; i < S * S; i += nt) tab[i] = a.log_trans[i];
    for (int j = tid; j < S; j += nt) prev[j] = lp[j] + a.log_p_init[j];
    __syncthreads();
    for (long long t = 1; t < a.T; ++t) {
        const double* lpt = lp + t * S;
        for (int j0 = 0; j0 < S; j0 += per_pass) {
            const int j = j0 + slot;
            const bool live = j < S;
            const double obs = live && sub == 0 ? lpt[j] : 0.0;  // (issued before the search, used after it)
            double best = vit_neg_inf();
            int bk = 0;
            if (live) {
                if (a.n_pred > 0) {
                    // eight candidates at a time, every load issued before the first use (one candidate per round trip to L2: 78 ms at pyin's shape; this: 55 ms)
                    const int n = a.pred_n[j];
                    const uint16_t* pk = a.pred_k + j;
                    const double* pl = a.pred_lt + j;
                    int e = sub;
                    for (; e + 7 * G < n; e += 8 * G) {
                        int k[8];
                        double l[8], v[8];
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            k[i] = pk[(long long)(e + i * G) * S];
                            l[i] = pl[(long long)(e + i * G) * S];
                        }
#pragma unroll
                        for (int i = 0; i < 8; ++i) v[i] = prev[k[i]];
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            const double c = v[i] + l[i];
                            if (c > best) { best = c; bk = k[i]; }
                        }
                    }
                    for (; e < n; e += G) {
                        const int k = pk[(long long)e * S];
                        const double c = prev[k] + pl[(long long)e * S];
                        if (c > best) { best = c; bk = k; }
                    }
                } else if (a.g.table_lds) {
                    for (int k = sub; k < S; k += G) {
                        const double c = prev[k] + tab[k * S + j];
                        if (c > best) { best = c; bk = k; }
                    }
                } else {
                    // (its own loop: one loop over either table would read both through flat addresses)
                    const double* lt = a.log_trans + j;
#pragma unroll 4
                    for (int k = sub; k < S; k += G) {
                        const double c = prev[k] + lt[(long long)k * S];
                        if (c > best) { best = c; bk = k; }
                    }
                }
            }
            for (int off = W; off < 64; off <<= 1) {
                const double oc = vit_shfl_xor(best, off);
                const int ok = vit_shfl_xor(bk, off);
                if (oc > best || (oc == best && ok < bk)) { best = oc; bk = ok; }
            }
            if (live && sub == 0) {
                cur[j] = obs + best;
                ptr[t * S + j] = (uint16_t)bk;
            }
        }
        __syncthreads();  // cur is complete, and nobody reads prev any more
        double* sw = prev;
        prev = cur;
        cur = sw;
    }
    double bv = 0.0;
    int bi = -1;
    for (int j = tid; j < S; j += nt)
        if (vit_argmax_better(prev[j], j, bv, bi)) { bv = prev[j]; bi = j; }
    red_v[tid] = bv;
    red_i[tid] = bi;
    __syncthreads();  // (also: every ptr store of the workgroup is visible to thread 0)
    if (tid == 0) {
        for (int i = 1; i < nt; ++i)
            if (vit_argmax_better(red_v[i], red_i[i], bv, bi)) { bv = red_v[i]; bi = red_i[i]; }
        uint16_t* st = a.states + chain * a.T;
        int s = bi;
        st[a.T - 1] = (uint16_t)s;
        for (long long t = a.T - 2; t >= 0; --t) {
            s = ptr[(t + 1) * S + s];
            st[t] = (uint16_t)s;
        }
        a.logp[chain] = bv;
    }
}

// grid = ceil(chains / (kSmallNT / g.lanes)) workgroups of kSmallNT threads; dynamic LDS = g.lds
__device__ __forceinline__ void small_body(const Args& a) {
    LRA_VIT_DYN_LDS(lds);
    const int S = a.S, G = a.g.lanes, tid = (int)threadIdx.x, grp = tid / G, sub = tid & (G - 1), base = (tid & 63) - sub;
    const long long chain = (long long)blockIdx.x * (kSmallNT / G) + grp;
    const bool chain_live = chain < a.chains, live = chain_live && sub < S;
    const long long table = chain_live ? chain % a.n_tables : 0;
    double* tab = reinterpret_cast<double*>(lds) + (long long)grp * S * S;
    if (chain_live)
        for (int i = sub; i < S * S; i += G) tab[i] = a.log_trans[table * S * S + i];
    __syncthreads();
    const double* lp = a.log_prob + (chain_live ? chain : 0) * a.T * S;
    uint16_t* ptr = a.ptr + (chain_live ? chain : 0) * a.T * S;
    double val = live ? lp[sub] + a.log_p_init[table * S + sub] : vit_neg_inf();
    for (long long t = 1; t < a.T; ++t) {
        const double obs = live ? lp[t * S + sub] : 0.0;
        double best = vit_neg_inf();
        int bk = 0;
        for (int k = 0; k < S; ++k) {
            const double vk = vit_shfl(val, base + k);
            if (live) {
                const double l = tab[k * S + sub];
                if (l >= a.threshold) {
                    const double c = vk + l;
                    if (c > best) { best = c; bk = k; }
                }
            }
        }
        val = obs + best;
        if (live) ptr[t * S + sub] = (uint16_t)bk;
    }
    double bv = val;
    int bi = live ? sub : -1;
    for (int off = 1; off < G; off <<= 1) {
        const double ov = vit_shfl_xor(bv, off);
        const int oi = vit_shfl_xor(bi, off);
        if (vit_argmax_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    __syncthreads();  // every ptr store of the group is visible to its first lane
    if (chain_live && sub == 0) {
        uint16_t* st = a.states + chain * a.T;
        int s = bi;
        st[a.T - 1] = (uint16_t)s;
        for (long long t = a.T - 2; t >= 0; --t) {
            s = ptr[(t + 1) * S + s];
            st[t] = (uint16_t)s;
        }
        a.logp[chain] = bv;
    }
}

// (plain functions, not templates: defined where LRA_VITERBI_KERNELS says so -- lra_viterbi_inst.hip and the simulator -- and nowhere else)
#if defined(LRA_VITERBI_KERNELS) || defined(LRA_POSTSIM)
__global__ __launch_bounds__(kPrepNT) void viterbi_prep(PrepArgs a) { prep_body(a); }
__global__ __launch_bounds__(kPrepNT) void viterbi_prep_binary(PrepArgs a) { prep_binary_body(a); }
__global__ __launch_bounds__(kWgMaxNT) void viterbi_wg(Args a) { wg_body(a); }
__global__ __launch_bounds__(kSmallNT) void viterbi_small(Args a) { small_body(a); }
#endif

}  // namespace viterbi
}  // namespace lra
