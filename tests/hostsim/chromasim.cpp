// chromasim.cpp -- runs the chroma kernel bodies of librosa_amd/csrc/lra_chroma.h on host fibres (tests/hostsim/simshim.h).
//
// TEST INFRASTRUCTURE ONLY.  Built by tests/hostsim_util.py (sim_lib) into tests/hostsim/_chromasim.so.
// Never linked into, imported by, or used as a fallback for the product library.
#define LRA_SIM_FIBRES 1
#include "simshim.h"

namespace lra {
namespace chroma {
double chroma_shfl_xor(double v, int offset) { return sim::wave_read(v, [=](unsigned me) { return me ^ (unsigned)offset; }); }
}  // namespace chroma
}  // namespace lra

#include "../../librosa_amd/csrc/lra_chroma.h"

extern "C" {
// which: 0 kFr, 1 kPass, 2 kTileF, 3 kColsF, 4 kRows, 5 / 6 the bins staged at a time for float / double
int chromasim_const(int which) {
    using namespace lra::chroma;
    const int v[] = {kFr, kPass, kTileF, kColsF, kRows, BinTile<float>::value, BinTile<double>::value};
    return v[which];
}

// the arguments of lra_chroma_exec (include/librosa_amd.h), host pointers; flag receives 1 when some raw value is not finite
int chromasim_exec(const void* x, long long batch, long long n_bins, long long n_frames, long long batch_stride, long long bin_stride, long long frame_stride, int is_f64, const void* w,
                   long long n_chroma, int norm, double threshold, int has_threshold, void* out, int* flag) {
    using namespace lra::chroma;
    *flag = 0;
    if (batch <= 0 || n_frames <= 0 || n_chroma <= 0) return 0;
    Args a{};
    a.x = x;
    a.batch_stride = batch_stride;
    a.bin_stride = bin_stride;
    a.frame_stride = frame_stride;
    a.n_bins = (int)n_bins;
    a.n_frames = n_frames;
    a.w = w;
    a.n_chroma = (int)n_chroma;
    a.norm = norm;
    a.has_thr = has_threshold != 0;
    a.thr = threshold;
    a.out = out;
    a.flag = flag;
    const bool rows = bin_stride == 1;
    const int per = rows ? kTileF : kColsF;
    a.tiles_per_clip = (n_frames + per - 1) / per;
    const unsigned grid = (unsigned)(a.tiles_per_clip * batch);
    if (rows) {
        if (is_f64) run_grid(grid, kNT, [=] { chroma_rows_kernel<double>(a); });
        else run_grid(grid, kNT, [=] { chroma_rows_kernel<float>(a); });
    } else {
        if (is_f64) run_grid(grid, kNT, [=] { chroma_cols_kernel<double>(a); });
        else run_grid(grid, kNT, [=] { chroma_cols_kernel<float>(a); });
    }
    return 0;
}
}
