// yinsim.cpp -- runs the YIN kernel bodies of librosa_amd/csrc/lra_yin.h on host threads (tests/hostsim/simshim.h), with the geometry and the
// twiddle tables of the library's own host functions (yin::prepare, mixed::fill_twiddles).
//
// TEST INFRASTRUCTURE ONLY.  Built by tests/hostsim_util.py (sim_lib) into tests/hostsim/_yinsim.so.
// Never linked into, imported by, or used as a fallback for the product library.
#define LRA_SIM_THREADS 1
#include "simshim.h"

namespace lra {
namespace yin {
double yin_shfl_up(double v, int delta) { return sim::wave_read(v, [=](unsigned me) { return (int)(me & 63u) >= delta ? me - (unsigned)delta : me; }); }
double yin_shfl_xor(double v, int offset) { return sim::wave_read(v, [=](unsigned me) { return me ^ (unsigned)offset; }); }
int yin_shfl_xor(int v, int offset) { return sim::wave_read(v, [=](unsigned me) { return me ^ (unsigned)offset; }); }
}  // namespace yin
}  // namespace lra

#include "../../librosa_amd/csrc/lra_yin.h"

namespace {
// every transform length of the device library, and the direct kernel
void run_yin(const lra::yin::Args& a, long long batch) {
    using namespace lra::yin;
    const unsigned grid = (unsigned)(batch * a.groups);
    switch (a.N) {
        case 0: run_grid(grid, kYinNT, [=] { yin_kernel<0>(a); }); break;
#define LRA_YIN_CASE(N) \
    case N: run_grid(grid, kYinNT, [=] { yin_kernel<N>(a); }); break;
        LRA_MIXED_SIZES(LRA_YIN_CASE)
#undef LRA_YIN_CASE
    }
}
}  // namespace

extern "C" {
// what lra_yin_exec decides for a geometry: out = {frames per workgroup, transform length (0: direct), frames per chunk, LDS bytes}
void yinsim_geometry(int W, int P, int* out) {
    using namespace lra::yin;
    Args a{};
    prepare(a, W, W, 1, 0, 0, 1, P, 0.0, 1.0, kF0);  // (one frame of any clip: the choice depends on W and P alone)
    out[0] = kYinGroup;
    out[1] = a.N;
    out[2] = a.N > 0 ? chunk_frames_of(a.N) : 1;
    out[3] = lds_layout(a.N, a.max_period).total;
}

// the arguments of lra_yin_exec (include/librosa_amd.h), host pointers; direct != 0 forces the direct kernel; returns -1 where the clip is too
// short, -2 where the LDS does not fit
int yinsim_exec(const void* y, long long batch, long long n, int is_f64, int W, int hop, int center, int pad_mode, int min_period, int max_period, double threshold, double sr, int mode,
                double* f0, void* frames, void* shifts, int direct) {
    using namespace lra::yin;
    Args a{};
    const int geometry = prepare(a, n, W, hop, center, pad_mode, min_period, max_period, threshold, sr, mode, direct != 0);
    if (geometry == lra::mixed::kGeometryTooShort) return -1;
    if (batch <= 0) return 0;
    if (geometry == lra::mixed::kGeometryLds) return -2;
    std::vector<cpx<double>> tw_m(a.N / 2 + 1), tw_n(a.N / 2 + 1);
    if (a.N > 0) lra::mixed::fill_twiddles<double>(a.N, tw_m.data(), tw_n.data());
    a.y = y;
    a.y_f64 = is_f64;
    a.tw_m = tw_m.data();
    a.tw_n = tw_n.data();
    a.f0 = f0;
    a.frames = frames;
    a.shifts = shifts;
    run_yin(a, batch);
    return 0;
}
}
