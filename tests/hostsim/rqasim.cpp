// rqasim.cpp -- runs the RQA kernel bodies of librosa_amd/csrc/lra_rqa.h on host fibres (tests/hostsim/simshim.h), with the launch geometry of
// the library's own host functions (rqa::geometry, rqa::argmax_parts) and its sequence of launches: one per block of rows.  The widening of an
// integer sim is lra_dtw.h's dtw_prepare, as in the library.
//
// TEST INFRASTRUCTURE ONLY.  Built by tests/hostsim_util.py (sim_lib) into tests/hostsim/_rqasim.so.
// Never linked into, imported by, or used as a fallback for the product library.
#define LRA_SIM_FIBRES 1
#include "simshim.h"

namespace lra {
namespace dtw {
void dtw_wave_sync() { sim::meet_wave(); }
void dtw_flag_or(int* word, int bits) { *word |= bits; }
}  // namespace dtw
}  // namespace lra

namespace lra {
namespace rqa {
void rqa_lds_sync() { sim::meet_block(); }
}  // namespace rqa
}  // namespace lra

#include "../../librosa_amd/csrc/lra_dtw.h"
#include "../../librosa_amd/csrc/lra_rqa.h"

extern "C" {
// out = {rows, strip, halo, width, nt, iters, lds}
void rqasim_geometry(int rows, int strip, int* out) {
    const lra::rqa::Geometry g = lra::rqa::geometry(rows, strip);
    out[0] = g.rows;
    out[1] = g.strip;
    out[2] = g.halo;
    out[3] = g.width;
    out[4] = g.nt;
    out[5] = g.iters;
    out[6] = g.lds;
}

int rqasim_served(int rows, int strip) { return (rows == 0 || lra::rqa::rows_ok(rows)) && (strip == 0 || lra::rqa::strip_ok(strip)); }

int rqasim_prepare(const void* in, int dtype, long long count, double* out) {
    using namespace lra::dtw;
    int flags = 0;
    PrepArgs a{in, dtype, count, out, &flags};
    run_grid_serial((unsigned)((count + kPrepNT - 1) / kPrepNT), kPrepNT, [=] { dtw_prepare(a); });
    return flags;
}

// the arguments of lra_rqa_score_exec, host pointers; returns the number of launches, -1 for a refused call
long long rqasim_score(const void* sim_, int is_f64, long long N, long long M, double gap_onset, double gap_extend, int knight, int rows, int strip, void* score, int8_t* pointers) {
    using namespace lra::rqa;
    if (N < 1 || M < 1 || !rqasim_served(rows, strip)) return -1;
    ScoreArgs a{};
    a.sim = sim_;
    a.f64 = is_f64;
    a.N = N;
    a.M = M;
    a.gap_onset = gap_onset;
    a.gap_extend = gap_extend;
    a.knight = knight != 0;
    a.score = score;
    a.ptr = pointers;
    a.g = geometry(rows, strip);
    const ScoreKernel kern = score_kernel(a.g.iters, a.f64);
    if (!kern) return -1;
    const unsigned grid = (unsigned)((M + a.g.strip - 1) / a.g.strip);
    long long launches = 0;
    for (long long row0 = 0; row0 < N; row0 += a.g.rows, ++launches) {
        a.row0 = row0;
        // the LDS of a launch holds nothing of the launch before it
        std::memset(g_postsim_dyn_lds, 0xA5, (size_t)a.g.lds);
        run_grid(grid, (unsigned)a.g.nt, [=] { kern(a); });
    }
    return launches;
}

// the arguments of lra_rqa_argmax_exec; returns the number of first-stage workgroups
int rqasim_argmax(const void* score, int is_f64, long long count, void* work) {
    using namespace lra::rqa;
    ArgmaxArgs a{};
    a.score = score;
    a.f64 = is_f64;
    a.count = count;
    a.out = (long long*)work;
    a.part_i = (long long*)((char*)work + 16);
    a.part_v = (double*)((char*)work + 16 + 8 * kMaxParts);
    a.parts = argmax_parts(count);
    run_grid((unsigned)a.parts, kArgNT, [=] { rqa_argmax_part(a); });
    run_grid(1, kArgNT, [=] { rqa_argmax_final(a); });
    return a.parts;
}

// the arguments of lra_rqa_backtrack_exec; returns the length
long long rqasim_backtrack(const int8_t* pointers, long long N, long long M, void* work, unsigned long long* path) {
    using namespace lra::rqa;
    BackArgs a{};
    a.ptr = pointers;
    a.N = N;
    a.M = M;
    a.start = (const long long*)work;
    a.path = path;
    a.cap = N < M ? N : M;
    a.length = (long long*)((char*)work + 8);
    run_grid(1, 64, [=] { rqa_backtrack(a); });
    return *a.length;
}
}
