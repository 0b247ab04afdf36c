// yinsim.cpp -- runs the YIN kernel bodies of librosa_amd/csrc/lra_yin.h on host threads.
//
// TEST INFRASTRUCTURE ONLY.  Built by tests/test_yin_host.py (g++ -DLRA_POSTSIM -pthread) into tests/hostsim/_yinsim.so.  One OS thread per
// lane of a workgroup, __syncthreads() is a barrier across them, the dynamic LDS is a static the lanes share; workgroups run one after the
// other.  Never linked into, imported by, or used as a fallback for the product library.
#define LRA_POSTSIM 1
#include <cmath>
#include <condition_variable>
#include <cstddef>
#include <mutex>
#include <thread>
#include <vector>

struct SimIdx { unsigned x = 0, y = 0, z = 0; };
static thread_local SimIdx threadIdx;
static thread_local SimIdx blockIdx;
static thread_local SimIdx blockDim;

namespace {
struct Barrier {
    std::mutex m;
    std::condition_variable cv;
    int n = 0, waiting = 0;
    unsigned long long gen = 0;
    void wait() {
        std::unique_lock<std::mutex> lk(m);
        const unsigned long long g = gen;
        if (++waiting == n) {
            waiting = 0;
            ++gen;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return gen != g; });
        }
    }
};
Barrier g_barrier;
}  // namespace
static inline void __syncthreads() { g_barrier.wait(); }

#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(...)
using std::exp;
using std::log;
using std::pow;
using std::sqrt;

// the wave shuffles of lra_yin.h: the 64 lanes of a wave meet at their own barrier and read each other's slot
namespace {
Barrier g_wave[4];
double g_slot[256];
int g_sloti[256];
}  // namespace
namespace lra {
namespace yin {
double yin_shfl_up(double v, int delta) {
    const unsigned me = threadIdx.x;
    g_slot[me] = v;
    g_wave[me >> 6].wait();
    const double r = (int)(me & 63u) >= delta ? g_slot[me - (unsigned)delta] : v;
    g_wave[me >> 6].wait();
    return r;
}
double yin_shfl_xor(double v, int offset) {
    const unsigned me = threadIdx.x;
    g_slot[me] = v;
    g_wave[me >> 6].wait();
    const double r = g_slot[me ^ (unsigned)offset];
    g_wave[me >> 6].wait();
    return r;
}
int yin_shfl_xor(int v, int offset) {
    const unsigned me = threadIdx.x;
    g_sloti[me] = v;
    g_wave[me >> 6].wait();
    const int r = g_sloti[me ^ (unsigned)offset];
    g_wave[me >> 6].wait();
    return r;
}
}  // namespace yin
}  // namespace lra

alignas(16) static unsigned char g_postsim_dyn_lds[160 * 1024];  // the dynamic LDS of the workgroup being run

#include "../../librosa_amd/csrc/lra_yin.h"

// the transform lengths of the device library (csrc/lra_mixed_launch.h), all instantiated here
#define LRA_MIXED_SIZES(X) X(160) X(200) X(240) X(320) X(400) X(480) X(600) X(640) X(720) X(800) X(882) X(960) X(1000) X(1200) X(1280) X(1440) X(1600) X(1764) X(1920) X(2000) X(2400) X(2646) X(3200) X(3528) X(4800)
static int sim_transform_length(int W, int P) {  // lra_yin_launch.h's transform_length
    int best = 0;
#define LRA_YIN_CASE(N) \
    if (N >= W + P && (best == 0 || N < best)) best = N;
    LRA_MIXED_SIZES(LRA_YIN_CASE)
#undef LRA_YIN_CASE
    return best;
}
using lra::mixed::cpx;
using lra::mixed::mkc;

namespace {
template <class F> void run_grid(unsigned grid, unsigned block, F body) {
    g_barrier.n = (int)block;
    for (auto& w : g_wave) w.n = 64;
    for (unsigned b = 0; b < grid; ++b) {
        std::vector<std::thread> lanes;
        for (unsigned t = 0; t < block; ++t)
            lanes.emplace_back([=] {
                threadIdx.x = t;
                blockIdx.x = b;
                blockDim.x = block;
                body();
            });
        for (auto& l : lanes) l.join();
    }
}

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
    const int N = sim_transform_length(W, P);
    out[0] = kYinGroup;
    out[1] = N;
    out[2] = N > 0 ? chunk_frames_of(N) : 1;
    out[3] = lds_layout(N, P).total;
}

// the arguments of lra_yin_exec (include/librosa_amd.h), host pointers; direct != 0 forces the direct kernel; returns -2 where the LDS does not fit
int yinsim_exec(const void* y, long long batch, long long n, int is_f64, int W, int hop, int center, int pad_mode, int min_period, int max_period, double threshold, double sr, int mode,
                double* f0, void* frames, void* shifts, int direct) {
    using namespace lra::yin;
    const int pad = center ? W / 2 : 0;
    if (n + 2 * (long long)pad < W) return -1;
    const long long n_frames = 1 + (n + 2 * (long long)pad - W) / hop;
    if (batch <= 0) return 0;
    Args a{};
    a.y = y;
    a.y_f64 = is_f64;
    a.n = n;
    a.n_frames = n_frames;
    a.W = W;
    a.hop = hop;
    a.pad = pad;
    a.pad_mode = pad_mode;
    a.N = direct ? 0 : sim_transform_length(W, max_period);
    a.min_period = min_period;
    a.max_period = max_period;
    a.threshold = threshold;
    a.sr = sr;
    a.tiny = 2.2250738585072014e-308;
    const int M = a.N / 2;
    const double two_pi = 6.283185307179586476925286766559;
    std::vector<cpx<double>> tw_m(M > 0 ? M : 1), tw_n(M + 1);  // as lra_api.hip's mixed_tables
    for (int t = 0; t < M; ++t) tw_m[t] = mkc<double>(std::cos(-two_pi * t / M), std::sin(-two_pi * t / M));
    for (int k = 0; k <= M; ++k) tw_n[k] = mkc<double>(std::cos(-two_pi * k / a.N), std::sin(-two_pi * k / a.N));
    a.tw_m = tw_m.data();
    a.tw_n = tw_n.data();
    a.mode = mode;
    a.f0 = f0;
    a.frames = frames;
    a.shifts = shifts;
    a.groups = (int)((n_frames + kYinGroup - 1) / kYinGroup);
    if (lds_layout(a.N, max_period).total > kYinLdsMax) return -2;
    run_yin(a, batch);
    return 0;
}
}
