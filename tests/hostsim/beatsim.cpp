// beatsim.cpp -- runs the beat-tracker kernel bodies of librosa_amd/csrc/lra_beat.h on host threads.
//
// TEST INFRASTRUCTURE ONLY.  Built by tests/test_beat_host.py (g++ -DLRA_POSTSIM -pthread) into tests/hostsim/_beatsim.so.  One OS thread per
// lane of a workgroup, __syncthreads() is a barrier across them, __shared__ is a static the lanes share; workgroups run one after the other.
// The kernel's cross-lane helpers (beat_wave_*) are stand-ins here: every lane posts its value, a barrier, every lane reads all of them.
// Never linked into, imported by, or used as a fallback for the product library.
#define LRA_POSTSIM 1
#include <cmath>
#include <condition_variable>
#include <cstddef>
#include <cstring>
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
double g_lane_d[64];
long long g_lane_ll[64];
}  // namespace
static inline void __syncthreads() { g_barrier.wait(); }

#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(...)
using std::exp;
using std::log;
using std::rint;
using std::sqrt;

namespace lra {
namespace beat {
double beat_wave_max(double v) {
    g_lane_d[threadIdx.x] = v;
    __syncthreads();
    double m = g_lane_d[0];
    for (int l = 1; l < 64; ++l) m = g_lane_d[l] > m ? g_lane_d[l] : m;
    __syncthreads();
    return m;
}
long long beat_wave_max_ll(long long v) {
    g_lane_ll[threadIdx.x] = v;
    __syncthreads();
    long long m = g_lane_ll[0];
    for (int l = 1; l < 64; ++l) m = g_lane_ll[l] > m ? g_lane_ll[l] : m;
    __syncthreads();
    return m;
}
long long beat_wave_sum_ll(long long v) {
    g_lane_ll[threadIdx.x] = v;
    __syncthreads();
    long long s = 0;
    for (int l = 0; l < 64; ++l) s += g_lane_ll[l];
    __syncthreads();
    return s;
}
unsigned long long beat_wave_ballot(int pred) {
    g_lane_ll[threadIdx.x] = pred != 0;
    __syncthreads();
    unsigned long long b = 0;
    for (int l = 0; l < 64; ++l) b |= (unsigned long long)(g_lane_ll[l] != 0) << l;
    __syncthreads();
    return b;
}
int beat_wave_read(int v, int lane) {
    g_lane_ll[threadIdx.x] = v;
    __syncthreads();
    const int r = (int)g_lane_ll[lane];
    __syncthreads();
    return r;
}
}  // namespace beat
}  // namespace lra

#include "../../librosa_amd/csrc/lra_beat.h"

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

template <class T> void run_all(const lra::beat::Args& a, long long batch) {
    using namespace lra::beat;
    run_grid((unsigned)batch, kBeatPrepNT, [=] { beat_prepare_kernel<T>(a); });
    run_grid((unsigned)(batch * ((a.n + 255) / 256)), 256, [=] { beat_local_score_kernel<T>(a); });
    run_grid((unsigned)batch, kBeatWave, [=] { beat_track_kernel<T>(a); });
}
}  // namespace

extern "C" {
// the arguments of lra_beat_exec (include/librosa_amd.h), host pointers; local / cum / backlink ([batch][n]: the envelope's type, float64,
// int32) receive the intermediate arrays
int beatsim_exec(const void* env, long long batch, long long n, int is_f64, const double* bpm, int bpm_mode, double frame_rate, double tightness, int trim, unsigned char* out,
                 void* local, double* cum, int* backlink, int* any_nonzero) {
    using namespace lra::beat;
    *any_nonzero = 0;
    if (batch <= 0 || n <= 0) return 0;
    const size_t cells = (size_t)batch * (size_t)n;
    std::vector<double> norm(cells), fpb(bpm_mode == kPerFrame ? cells : (size_t)batch);
    std::vector<int> order(cells), dead((size_t)batch);
    Args a{};
    a.env = env;
    a.n = n;
    a.bpm = bpm;
    a.bpm_mode = bpm_mode;
    a.frame_rate = frame_rate;
    a.tightness = (float)tightness;
    a.trim = trim != 0;
    a.norm = norm.data();
    a.local = local;
    a.fpb = fpb.data();
    a.cum = cum;
    a.backlink = backlink;
    a.order = order.data();
    a.dead = dead.data();
    a.any = any_nonzero;
    a.out = out;
    if (is_f64) run_all<double>(a, batch);
    else run_all<float>(a, batch);
    return 0;
}
}
