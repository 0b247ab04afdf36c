// dtwsim.cpp -- runs the DTW kernel bodies of librosa_amd/csrc/lra_dtw.h on host fibres (tests/hostsim/simshim.h), with the launch geometry of
// the library's own host functions (dtw::geometry, dtw::diag_tiles) and its sequence of launches: one per tile anti-diagonal.
//
// TEST INFRASTRUCTURE ONLY.  Built by tests/hostsim_util.py (sim_lib) into tests/hostsim/_dtwsim.so.
// Never linked into, imported by, or used as a fallback for the product library.
#define LRA_SIM_FIBRES 1
#include "simshim.h"

namespace lra {
namespace dtw {
void dtw_wave_sync() { sim::meet_wave(); }
void dtw_flag_or(int* word, int bits) { *word |= bits; }
}  // namespace dtw
}  // namespace lra

#include "../../librosa_amd/csrc/lra_dtw.h"

namespace {
bool step_table(const int* steps, const double* w_add, const double* w_mul, int n_steps, lra::dtw::StepTable* st) {
    using namespace lra::dtw;
    if (n_steps < 1 || n_steps > kMaxSteps) return false;
    *st = StepTable{};
    st->n = n_steps;
    for (int i = 0; i < n_steps; ++i) {
        const int s0 = steps[2 * i], s1 = steps[2 * i + 1];
        if (s0 < 0 || s1 < 0 || s0 > kMaxStep || s1 > kMaxStep || (s0 == 0 && s1 == 0)) return false;
        st->s0[i] = s0;
        st->s1[i] = s1;
        st->w_add[i] = w_add ? w_add[i] : 0.0;
        st->w_mul[i] = w_mul ? w_mul[i] : 1.0;
        if (s0 > st->max0) st->max0 = s0;
        if (s1 > st->max1) st->max1 = s1;
    }
    return true;
}
}  // namespace

extern "C" {
// out = {tile, d_rows, d_stride, off_c, off_s, lds}
void dtwsim_geometry(int tile, int max0, int max1, int* out) {
    const lra::dtw::Geometry g = lra::dtw::geometry(tile, max0, max1);
    out[0] = g.tile;
    out[1] = g.d_rows;
    out[2] = g.d_stride;
    out[3] = g.off_c;
    out[4] = g.off_s;
    out[5] = g.lds;
}

// the arguments of lra_dtw_cost_exec (include/librosa_amd.h), host pointers; returns the flags
int dtwsim_cost(const void* X, const void* Y, int is_f64, long long K, long long N, long long M, int metric, double* C) {
    using namespace lra::dtw;
    int flags = 0;
    CostArgs a{X, Y, is_f64, metric, K, N, M, C, &flags};
    const long long grid = ((N + kCostTile - 1) / kCostTile) * ((M + kCostTile - 1) / kCostTile);
    run_grid((unsigned)grid, kCostNT, [=] { dtw_cost(a); });
    return flags;
}

int dtwsim_prepare(const void* C, int dtype, long long count, double* out) {
    using namespace lra::dtw;
    int flags = 0;
    PrepArgs a{C, dtype, count, out, &flags};
    run_grid_serial((unsigned)((count + kPrepNT - 1) / kPrepNT), kPrepNT, [=] { dtw_prepare(a); });
    return flags;
}

// the arguments of lra_dtw_accumulate_exec; returns the number of launches, -1 for a refused call
long long dtwsim_accumulate(const double* C, long long N, long long M, const int* steps, const double* w_add, const double* w_mul, int n_steps, int subseq, int band, long long band_lo,
                            long long band_hi, int tile, double* D, uint8_t* step_idx) {
    using namespace lra::dtw;
    AccArgs a{};
    if (!step_table(steps, w_add, w_mul, n_steps, &a.st) || (tile != 0 && !tile_ok(tile)) || N < 1 || M < 1) return -1;
    a.C = C;
    a.N = N;
    a.M = M;
    a.subseq = subseq;
    a.band = band;
    a.band_lo = band_lo;
    a.band_hi = band_hi;
    a.D = D;
    a.steps = step_idx;
    a.g = geometry(tile, a.st.max0, a.st.max1);
    if (a.g.lds > kLdsMax) return -1;
    a.tiles_n = (N + a.g.tile - 1) / a.g.tile;
    a.tiles_m = (M + a.g.tile - 1) / a.g.tile;
    long long launches = 0;
    for (long long diag = 0; diag < a.tiles_n + a.tiles_m - 1; ++diag, ++launches) {
        a.diag = diag;
        // the LDS of a tile holds nothing of the tile before it
        std::memset(g_postsim_dyn_lds, 0xA5, (size_t)a.g.lds);
        const unsigned grid = (unsigned)diag_tiles(diag, a.tiles_n, a.tiles_m).count;
        if (a.st.n == 3) run_grid(grid, kAccNT, [=] { dtw_accumulate(a); });
        else run_grid(grid, kAccNT, [=] { dtw_accumulate_any(a); });
    }
    return launches;
}

void dtwsim_widen(const uint8_t* in, long long count, int* out) {
    using namespace lra::dtw;
    WidenArgs a{in, count, out};
    run_grid_serial((unsigned)((count + kPrepNT - 1) / kPrepNT), kPrepNT, [=] { dtw_widen(a); });
}

// the arguments of lra_dtw_backtrack_exec; returns the status, -1 for a refused call
int dtwsim_backtrack(const double* D, const void* step_idx, int steps_i32, long long N, long long M, const int* steps, int n_steps, int subseq, long long start, long long* path,
                     long long* length) {
    using namespace lra::dtw;
    BackArgs a{};
    if (!step_table(steps, nullptr, nullptr, n_steps, &a.st) || N < 1 || M < 1 || start < kStartArgmin || start >= M || (start == kStartArgmin && !D)) return -1;
    int status = 0;
    a.D = D;
    a.steps = step_idx;
    a.steps_i32 = steps_i32;
    a.N = N;
    a.M = M;
    a.subseq = subseq;
    a.start = start;
    a.path = path;
    a.cap = N + M - 1;
    a.length = length;
    a.status = &status;
    run_grid(1, kBackNT, [=] { dtw_backtrack(a); });
    return status;
}
}
