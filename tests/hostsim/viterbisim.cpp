// viterbisim.cpp -- runs the Viterbi kernel bodies of librosa_amd/csrc/lra_viterbi.h on host fibres (tests/hostsim/simshim.h), with the launch
// geometry of the library's own host function (viterbi::geometry).
//
// TEST INFRASTRUCTURE ONLY.  Built by tests/hostsim_util.py (sim_lib) into tests/hostsim/_viterbisim.so.
// Never linked into, imported by, or used as a fallback for the product library.
#define LRA_SIM_FIBRES 1
#include "simshim.h"

namespace lra {
namespace viterbi {
double vit_shfl(double v, int lane) { return sim::wave_read(v, [=](unsigned me) { return (me & ~63u) + (unsigned)lane; }); }
double vit_shfl_xor(double v, int offset) { return sim::wave_read(v, [=](unsigned me) { return me ^ (unsigned)offset; }); }
int vit_shfl_xor(int v, int offset) { return sim::wave_read(v, [=](unsigned me) { return me ^ (unsigned)offset; }); }
void vit_flag_or(int* word, int bits) { *word |= bits; }
}  // namespace viterbi
}  // namespace lra

#include "../../librosa_amd/csrc/lra_viterbi.h"

extern "C" {
// what lra_viterbi_exec decides for a size: out = {small kernel, threads, lanes per target or chain, table in LDS, LDS bytes}
void viterbisim_geometry(int n_states, int n_pred, int* out) {
    const lra::viterbi::Geometry g = lra::viterbi::geometry(n_states, n_pred);
    out[0] = g.small;
    out[1] = g.nt;
    out[2] = g.lanes;
    out[3] = g.table_lds;
    out[4] = g.lds;
}

// the arguments of lra_viterbi_prep_exec (include/librosa_amd.h), host pointers; returns the flags
int viterbisim_prep(const void* prob, int is_f64, int kind, long long chains, int n_states, long long n_steps, double eps, const double* log_marginal, int n_labels, double* log_prob) {
    using namespace lra::viterbi;
    int flags = 0;
    PrepArgs a{prob, is_f64, kind, chains, n_states, n_steps, eps, log_marginal, n_labels > 0 ? n_labels : 1, log_prob, &flags};
    if (chains <= 0 || n_steps <= 0) return 0;
    if (kind == kBinary) run_grid((unsigned)((chains * n_steps + kPrepNT - 1) / kPrepNT), kPrepNT, [=] { viterbi_prep_binary(a); });
    else run_grid((unsigned)(chains * ((n_steps + kPrepSteps - 1) / kPrepSteps)), kPrepNT, [=] { viterbi_prep(a); });
    return flags;
}

// the arguments of lra_viterbi_exec, host pointers; returns -1 where the LDS does not fit
int viterbisim_exec(const double* log_prob, long long chains, int n_states, long long n_steps, const double* log_trans, const double* log_p_init, int n_tables, double threshold, int n_pred,
                    const uint16_t* pred_k, const double* pred_lt, const int* pred_n, uint16_t* ptr, uint16_t* states, double* logp) {
    using namespace lra::viterbi;
    if (n_states > kMaxStates) return -1;
    Args a{};
    a.log_prob = log_prob;
    a.log_trans = log_trans;
    a.log_p_init = log_p_init;
    a.n_tables = n_tables;
    a.chains = chains;
    a.S = n_states;
    a.T = n_steps;
    a.threshold = threshold;
    a.n_pred = n_states > kSmallMax ? n_pred : 0;
    a.pred_k = pred_k;
    a.pred_lt = pred_lt;
    a.pred_n = pred_n;
    a.ptr = ptr;
    a.states = states;
    a.logp = logp;
    a.g = geometry(n_states, a.n_pred);
    if (a.g.lds > kLdsMax) return -1;
    if (chains <= 0) return 0;
    if (a.g.small) run_grid((unsigned)((chains + kSmallNT / a.g.lanes - 1) / (kSmallNT / a.g.lanes)), kSmallNT, [=] { viterbi_small(a); });
    else run_grid((unsigned)chains, (unsigned)a.g.nt, [=] { viterbi_wg(a); });
    return 0;
}
}
