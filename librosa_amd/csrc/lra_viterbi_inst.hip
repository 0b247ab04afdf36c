// lra_viterbi_inst.hip -- the Viterbi kernels (lra_viterbi.h) and their launchers and the C entry points they serve, a translation unit of its own so
// that it compiles side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#define LRA_VITERBI_KERNELS 1
#include "lra_viterbi.h"

#include "lra_internal.h"

namespace lra {
namespace viterbi {

hipError_t launch_prep(const PrepArgs& a, hipStream_t stream) {
    if (a.clips <= 0 || a.T <= 0 || a.S <= 0) return hipSuccess;
    const long long grid = a.kind == kBinary ? (a.clips * a.T + kPrepNT - 1) / kPrepNT : a.clips * ((a.T + kPrepSteps - 1) / kPrepSteps);
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    if (a.kind == kBinary) hipLaunchKernelGGL(viterbi_prep_binary, dim3((unsigned)grid), dim3(kPrepNT), 0, stream, a);
    else hipLaunchKernelGGL(viterbi_prep, dim3((unsigned)grid), dim3(kPrepNT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_decode(const Args& a, hipStream_t stream) {
    if (a.chains <= 0 || a.T <= 0) return hipSuccess;
    const Geometry& g = a.g;
    if (g.lds > kLdsMax || g.nt > kWgMaxNT) return hipErrorInvalidConfiguration;
    const long long grid = g.small ? (a.chains + kSmallNT / g.lanes - 1) / (kSmallNT / g.lanes) : a.chains;
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    void (*kern)(Args) = g.small ? viterbi_small : viterbi_wg;
    if (g.lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, g.lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(g.nt), g.lds, stream, a);
    return hipGetLastError();
}

}  // namespace viterbi
}  // namespace lra

// ---- C entry points: sequence.viterbi and its variants -------------------------------------------------------------------------------------------
using namespace lra;

extern "C" {

static_assert(viterbi::kGenerative == LRA_VITERBI_GENERATIVE && viterbi::kDiscriminative == LRA_VITERBI_DISCRIMINATIVE && viterbi::kBinary == LRA_VITERBI_BINARY &&
                  viterbi::kLog == LRA_VITERBI_LOG,
              "viterbi kinds");
static_assert(viterbi::kFlagNegative == LRA_VITERBI_FLAG_NEGATIVE && viterbi::kFlagAboveOne == LRA_VITERBI_FLAG_ABOVE_ONE && viterbi::kFlagColumnSum == LRA_VITERBI_FLAG_COLUMN_SUM,
              "viterbi flags");
static_assert(viterbi::kMaxStates == LRA_VITERBI_MAX_STATES && viterbi::kSmallMax == LRA_VITERBI_SMALL_MAX && viterbi::kLdsMax == LRA_VITERBI_LDS_MAX, "viterbi limits");
static_assert(viterbi::geometry(viterbi::kMaxStates, 0).lds <= viterbi::kLdsMax && viterbi::geometry(viterbi::kMaxStates, 1).lds <= viterbi::kLdsMax, "viterbi: the largest call fits");

int64_t lra_viterbi_lds_bytes(int n_states, int n_pred) {
    if (n_states < 1) return 0;
    if (n_states > viterbi::kMaxStates) return (int64_t)viterbi::kLdsMax + 16LL * (n_states - viterbi::kMaxStates);  // (refused: the limit is a round number below what the LDS holds)
    return viterbi::geometry(n_states, n_pred > 0 ? n_pred : 0).lds;
}

int lra_viterbi_prep_exec(lra_ctx* ctx, const void* prob, int dtype, int kind, int64_t chains, int n_states, int64_t n_steps, double eps, const void* log_marginal, int n_labels,
                          void* log_prob, void* work, int* flags) {
    LRA_BIND(ctx);
    if (flags) *flags = 0;
    if (kind < LRA_VITERBI_GENERATIVE || kind > LRA_VITERBI_LOG) return fail(LRA_EINVAL, "viterbi: unknown kind");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "viterbi: dtype must be LRA_F32 or LRA_F64");
    if (chains < 0 || n_steps < 0 || n_states < 1) return fail(LRA_EINVAL, "viterbi: negative size");
    if (kind == LRA_VITERBI_BINARY && (n_states != 2 || n_labels < 1)) return fail(LRA_EINVAL, "viterbi: a binary chain has 2 states and at least one label");
    if (chains == 0 || n_steps == 0) return LRA_OK;
    if (!prob || !log_prob || !work) return fail(LRA_EINVAL, "null data pointer");
    if ((kind == LRA_VITERBI_DISCRIMINATIVE || kind == LRA_VITERBI_BINARY) && !log_marginal) return fail(LRA_EINVAL, "viterbi: log_marginal is missing");
    viterbi::PrepArgs a{};
    a.prob = prob;
    a.f64 = dtype == LRA_F64;
    a.kind = kind;
    a.clips = chains;
    a.S = n_states;
    a.T = n_steps;
    a.eps = eps;
    a.log_marginal = (const double*)log_marginal;
    a.n_labels = n_labels > 0 ? n_labels : 1;
    a.log_prob = (double*)log_prob;
    a.flags = (int*)work;
    LRA_HIP(hipMemsetAsync(work, 0, sizeof(int), ctx->stream));
    LRA_HIP(viterbi::launch_prep(a, ctx->stream));
    if (flags) {
        int h = 0;
        LRA_TRY(read_status(ctx, work, &h, sizeof(h)));
        *flags = h;
    }
    return LRA_OK;
}

int lra_viterbi_exec(lra_ctx* ctx, const void* log_prob, int64_t chains, int n_states, int64_t n_steps, const void* log_trans, const void* log_p_init, int n_tables, double threshold,
                     int n_pred, const void* pred_k, const void* pred_lt, const void* pred_n, void* ptr, void* states, void* logp) {
    LRA_BIND(ctx);
    if (chains < 0 || n_steps < 1 || n_states < 1 || n_tables < 1 || n_pred < 0) return fail(LRA_EINVAL, "viterbi: need n_states, n_steps and n_tables of at least 1");
    if (n_states > viterbi::kMaxStates)
        return fail(LRA_EINVAL, "viterbi: n_states=" + std::to_string(n_states) + " does not fit the LDS of a workgroup (at most " + std::to_string(viterbi::kMaxStates) + ")");
    if (threshold != threshold) return fail(LRA_EINVAL, "viterbi: threshold is NaN");
    const bool small = n_states <= viterbi::kSmallMax, listed = !small && threshold > -HUGE_VAL;
    if (!small && n_tables != 1) return fail(LRA_EINVAL, "viterbi: a table per chain is served up to " + std::to_string(viterbi::kSmallMax) + " states");
    if (listed && (n_pred < 1 || n_pred > n_states)) return fail(LRA_EINVAL, "viterbi: a thresholded search needs predecessor lists of 1 to n_states rows");
    if (chains == 0) return LRA_OK;
    if (!log_prob || !log_p_init || !ptr || !states || !logp || (!listed && !log_trans) || (listed && (!pred_k || !pred_lt || !pred_n))) return fail(LRA_EINVAL, "null data pointer");
    viterbi::Args a{};
    a.log_prob = (const double*)log_prob;
    a.log_trans = (const double*)log_trans;
    a.log_p_init = (const double*)log_p_init;
    a.n_tables = n_tables;
    a.chains = chains;
    a.S = n_states;
    a.T = n_steps;
    a.threshold = threshold;
    a.n_pred = listed ? n_pred : 0;
    a.pred_k = (const uint16_t*)pred_k;
    a.pred_lt = (const double*)pred_lt;
    a.pred_n = (const int*)pred_n;
    a.ptr = (uint16_t*)ptr;
    a.states = (uint16_t*)states;
    a.logp = (double*)logp;
    a.g = viterbi::geometry(n_states, a.n_pred);
    LRA_HIP(viterbi::launch_decode(a, ctx->stream));
    return LRA_OK;
}

}  // extern "C"
