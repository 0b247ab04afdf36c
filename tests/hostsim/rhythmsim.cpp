// rhythmsim.cpp -- runs the tempogram / tempo kernel bodies of librosa_amd/csrc/lra_rhythm.h on host threads (tests/hostsim/simshim.h), with
// the geometry and the twiddle tables of the library's own host functions (rhythm::prepare, mixed::fill_twiddles).
//
// TEST INFRASTRUCTURE ONLY.  Built by tests/hostsim_util.py (sim_lib) into tests/hostsim/_rhythmsim.so.
// Never linked into, imported by, or used as a fallback for the product library.
#define LRA_SIM_THREADS 1
#include "simshim.h"

#include "../../librosa_amd/csrc/lra_rhythm.h"

namespace {
// the kernel of lra_tempogram_exec's choice: every transform length of the device library, and the direct sum
void run_tempogram(const lra::rhythm::Args& a, long long batch) {
    using namespace lra::rhythm;
    const unsigned grid = (unsigned)(batch * a.groups);
    switch (a.N) {
        case 0: run_grid(grid, kRhythmNT, [=] { tempogram_kernel<0>(a); }); break;
#define LRA_RHYTHM_CASE(N) \
    case N: run_grid(grid, kRhythmNT, [=] { tempogram_kernel<N>(a); }); break;
        LRA_MIXED_SIZES(LRA_RHYTHM_CASE)
#undef LRA_RHYTHM_CASE
    }
}
}  // namespace

extern "C" {
// what lra_tempogram_exec decides for a window length and a mode: out = {transform length (0: direct), tile, LDS bytes of that choice}
void rhythmsim_geometry(int W, int mode, int* out) {
    using namespace lra::rhythm;
    Args a{};
    prepare(a, W, W, 0, kNormInf, mode);  // (one frame of any envelope: the choice depends on W and the mode alone)
    out[0] = a.N;
    out[1] = a.tile;
    out[2] = lds_layout(a.N, W, mode, a.tile != 0).total;
}

// the arguments of lra_tempogram_exec (include/librosa_amd.h), host pointers; direct != 0 forces the O(W^2) kernel; returns -2 where the LDS
// does not fit
int rhythmsim_exec(const void* env, long long batch, long long n, int is_f64, int W, int center, const double* window, int norm, int mode, const double* logprior,
                   const double* bpms, double* out, int direct, int* nonfinite) {
    using namespace lra::rhythm;
    *nonfinite = 0;
    Args a{};
    const int geometry = prepare(a, n, W, center, norm, mode, direct != 0);
    if (geometry == lra::mixed::kGeometryTooShort || batch <= 0 || a.n_frames <= 0) return 0;
    if (geometry == lra::mixed::kGeometryLds) return -2;
    std::vector<cpx<double>> tw_m(a.N / 2 + 1), tw_n(a.N / 2 + 1);
    if (a.N > 0) lra::mixed::fill_twiddles<double>(a.N, tw_m.data(), tw_n.data());
    std::vector<double> partial(mode == kSum ? (size_t)batch * a.groups * W : 1);
    int flag = 0;
    a.env = env;
    a.env_f64 = is_f64;
    a.win = window;
    a.tw_m = tw_m.data();
    a.tw_n = tw_n.data();
    a.logprior = logprior;
    a.bpms = bpms;
    a.out = out;
    a.partial = partial.data();
    a.flag = &flag;
    run_tempogram(a, batch);
    if (mode == kSum) {
        FinishArgs f{a.partial, logprior, bpms, out, a.n_frames, a.groups, W};
        run_grid((unsigned)batch, 256, [=] { tempo_mean_finish_kernel<double>(f); });
    }
    *nonfinite = flag;
    return 0;
}
}
