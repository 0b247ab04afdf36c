// chromasim.cpp -- runs the chroma kernel bodies of librosa_amd/csrc/lra_chroma.h on the host.
//
// TEST INFRASTRUCTURE ONLY.  Built by tests/test_chroma_host.py (g++ -DLRA_POSTSIM) into tests/hostsim/_chromasim.so.  One fibre (ucontext) per
// lane of a workgroup, all on the calling thread and resumed in lane order: __syncthreads() hands control back to the scheduler, so one sweep
// over the fibres is one barrier phase (the kernels reach their barriers uniformly); __shared__ is a static the lanes share; workgroups run
// one after the other.  The wave exchange is a stand-in: every lane posts its value, a sweep, every lane reads its partner's, a sweep.
// Never linked into, imported by, or used as a fallback for the product library.
#define LRA_POSTSIM 1
#include <ucontext.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

struct SimIdx { unsigned x = 0, y = 0, z = 0; };
static SimIdx threadIdx;
static SimIdx blockIdx;
static SimIdx blockDim;

namespace {
struct Fibre {
    ucontext_t ctx;
    std::vector<char> stack;
    bool done = false;
};
ucontext_t g_sched;
std::vector<Fibre> g_fibres;
Fibre* g_cur = nullptr;
unsigned g_lane = 0;  // the running fibre's thread index (threadIdx.x is only valid until the first hand-over)
std::function<void()> g_body;
double g_slot[1024];

void fibre_main() {
    g_body();
    g_cur->done = true;
}
void hand_over() { swapcontext(&g_cur->ctx, &g_sched); }
}  // namespace
static inline void __syncthreads() { hand_over(); }

#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(...)

namespace lra {
namespace chroma {
double chroma_shfl_xor(double v, int offset) {
    const unsigned me = g_lane;
    g_slot[me] = v;
    hand_over();
    const double r = g_slot[me ^ (unsigned)offset];
    hand_over();
    return r;
}
}  // namespace chroma
}  // namespace lra

#include "../../librosa_amd/csrc/lra_chroma.h"

namespace {
template <class F> void run_grid(unsigned grid, unsigned block, F body) {
    g_body = body;
    g_fibres.resize(block);
    for (auto& f : g_fibres) f.stack.resize(256 * 1024);
    for (unsigned b = 0; b < grid; ++b) {
        for (unsigned t = 0; t < block; ++t) {
            Fibre& f = g_fibres[t];
            f.done = false;
            getcontext(&f.ctx);
            f.ctx.uc_stack.ss_sp = f.stack.data();
            f.ctx.uc_stack.ss_size = f.stack.size();
            f.ctx.uc_link = &g_sched;
            makecontext(&f.ctx, fibre_main, 0);
        }
        bool live = true;
        bool first = true;
        while (live) {
            live = false;
            for (unsigned t = 0; t < block; ++t) {
                Fibre& f = g_fibres[t];
                if (f.done) continue;
                g_cur = &f;
                g_lane = t;
                if (first) {
                    threadIdx.x = t;
                    blockIdx.x = b;
                    blockDim.x = block;
                }
                swapcontext(&g_sched, &f.ctx);
                live = live || !f.done;
            }
            first = false;
        }
    }
}
}  // namespace

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
