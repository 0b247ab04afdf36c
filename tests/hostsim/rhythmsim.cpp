// rhythmsim.cpp -- runs the tempogram / tempo kernel bodies of librosa_amd/csrc/lra_rhythm.h on host threads.
//
// TEST INFRASTRUCTURE ONLY.  Built by tests/test_rhythm_host.py (g++ -DLRA_POSTSIM -pthread) into tests/hostsim/_rhythmsim.so.  One OS
// thread per lane of a workgroup, __syncthreads() is a barrier across them, __shared__ is a static the lanes share; workgroups run one
// after the other.  Never linked into, imported by, or used as a fallback for the product library.
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
using std::expm1;
using std::log;
using std::log10;
using std::log1p;
using std::pow;
using std::sqrt;

alignas(16) static unsigned char g_postsim_dyn_lds[160 * 1024];  // the dynamic LDS of the workgroup being run

#include "../../librosa_amd/csrc/lra_rhythm.h"

// transform lengths instantiated here: every size of LRA_MIXED_SIZES, as the device library (tests/test_rhythm_edges_host.py runs them all);
// sim_transform_length is lra_rhythm_launch.h's transform_length over the full list, -1 where its choice is not instantiated here
#define LRA_MIXED_SIZES(X) X(160) X(200) X(240) X(320) X(400) X(480) X(600) X(640) X(720) X(800) X(882) X(960) X(1000) X(1200) X(1280) X(1440) X(1600) X(1764) X(1920) X(2000) X(2400) X(2646) X(3200) X(3528) X(4800)
#define LRA_RHYTHM_SIM_SIZES(X) LRA_MIXED_SIZES(X)
static int sim_transform_length(int W) {
    int best = 0;
#define LRA_RHYTHM_CASE(N) \
    if (N >= 2 * W - 1 && (best == 0 || N < best)) best = N;
    LRA_MIXED_SIZES(LRA_RHYTHM_CASE)
#undef LRA_RHYTHM_CASE
    bool ok = best == 0;
#define LRA_RHYTHM_CASE(N) ok |= best == N;
    LRA_RHYTHM_SIM_SIZES(LRA_RHYTHM_CASE)
#undef LRA_RHYTHM_CASE
    return ok ? best : -1;
}
using lra::mixed::cpx;
using lra::mixed::mkc;

namespace {
template <class F> void run_grid(unsigned grid, unsigned block, F body) {
    g_barrier.n = (int)block;
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

// the kernel of lra_tempogram_exec's choice (transform length from the size list, or the direct sum)
void run_tempogram(const lra::rhythm::Args& a, long long batch) {
    using namespace lra::rhythm;
    const unsigned grid = (unsigned)(batch * a.groups);
    switch (a.N) {
        case 0: run_grid(grid, kRhythmNT, [=] { tempogram_kernel<0>(a); }); break;
#define LRA_RHYTHM_CASE(N) \
    case N: run_grid(grid, kRhythmNT, [=] { tempogram_kernel<N>(a); }); break;
        LRA_RHYTHM_SIM_SIZES(LRA_RHYTHM_CASE)
#undef LRA_RHYTHM_CASE
    }
}
}  // namespace

extern "C" {
// the arguments of lra_tempogram_exec (include/librosa_amd.h), host pointers; direct != 0 forces the O(W^2) kernel; returns -1 for a
// transform length this simulator does not instantiate
int rhythmsim_exec(const void* env, long long batch, long long n, int is_f64, int W, int center, const double* window, int norm, int mode, const double* logprior,
                   const double* bpms, double* out, int direct, int* nonfinite) {
    using namespace lra::rhythm;
    *nonfinite = 0;
    const int pad = center ? W / 2 : 0;
    const long long n_frames = center ? n : n - W + 1;
    if (batch <= 0 || n_frames <= 0) return 0;
    Args a{};
    a.env = env;
    a.env_f64 = is_f64;
    a.n = n;
    a.n_frames = n_frames;
    a.W = W;
    a.pad = pad;
    a.N = direct ? 0 : sim_transform_length(W);
    if (a.N < 0) return -1;
    const int M = a.N / 2;
    const double two_pi = 6.283185307179586476925286766559;
    std::vector<cpx<double>> tw_m(M > 0 ? M : 1), tw_n(M + 1);  // as lra_api.hip's mixed_tables
    for (int t = 0; t < M; ++t) tw_m[t] = mkc<double>(std::cos(-two_pi * t / M), std::sin(-two_pi * t / M));
    for (int k = 0; k <= M; ++k) tw_n[k] = mkc<double>(std::cos(-two_pi * k / a.N), std::sin(-two_pi * k / a.N));
    a.win = window;
    a.tw_m = tw_m.data();
    a.tw_n = tw_n.data();
    a.norm = norm;
    a.mode = mode;
    a.tile = mode == kWrite && lds_layout(a.N, W, mode, true).total <= kRhythmLdsMax;
    a.logprior = logprior;
    a.bpms = bpms;
    a.out = out;
    a.groups = (int)((n_frames + kRhythmGroup - 1) / kRhythmGroup);
    std::vector<double> partial(mode == kSum ? (size_t)batch * a.groups * W : 1);
    int flag = 0;
    a.partial = partial.data();
    a.flag = &flag;
    if (lds_layout(a.N, W, mode, false).total > kRhythmLdsMax) return -2;
    run_tempogram(a, batch);
    if (mode == kSum) {
        FinishArgs f{a.partial, logprior, bpms, out, n_frames, a.groups, W};
        run_grid((unsigned)batch, 256, [=] { tempo_mean_finish_kernel<double>(f); });
    }
    *nonfinite = flag;
    return 0;
}
}
