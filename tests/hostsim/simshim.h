// simshim.h -- the lane shim of the host simulators (postsim, onsetsim, rhythmsim, beatsim, peaksim, yinsim, chromasim, pitchsim): what a
// kernel header of librosa_amd/csrc needs in place of <hip/hip_runtime.h> to run its kernel bodies on the CPU.
//
// TEST INFRASTRUCTURE ONLY.  Never linked into, imported by, or used as a fallback for the product library.
//
// A simulator defines ONE of the two scheduler macros, includes this file, then its kernel header:
//   LRA_SIM_THREADS  one OS thread per lane of a workgroup (build with -pthread); __syncthreads() is a barrier across them.
//   LRA_SIM_FIBRES   one fibre (ucontext) per lane, all on the calling thread and resumed in lane order; __syncthreads() hands control back
//                    to the scheduler, so one sweep over the fibres is one barrier phase (the kernels reach their barriers uniformly).
// Either way __shared__ is a static the lanes share, the dynamic LDS is g_postsim_dyn_lds, workgroups run one after the other, and
// threadIdx / blockIdx / blockDim / gridDim (.x only) hold the running lane's values whenever kernel code runs.
//
// The cross-lane instructions are stand-ins on a slot array (sim::wave_read / wave_reduce / wave_ballot below): every lane posts its value,
// the wave meets, every lane reads what it wants of the others', the wave meets again.  A simulator writes the names its kernel header
// expects (yin_shfl_xor, beat_wave_max, pitch_ballot, ...) as one-line calls of these.
#pragma once
#define LRA_POSTSIM 1
#if defined(LRA_SIM_THREADS) == defined(LRA_SIM_FIBRES)
#error "define exactly one of LRA_SIM_THREADS and LRA_SIM_FIBRES before including simshim.h"
#endif

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>
#ifdef LRA_SIM_THREADS
#include <condition_variable>
#include <mutex>
#include <thread>
#define LRA_SIM_PER_LANE thread_local
#else
#include <ucontext.h>

#include <functional>
#define LRA_SIM_PER_LANE
#endif

struct SimIdx { unsigned x = 0, y = 0, z = 0; };
static LRA_SIM_PER_LANE SimIdx threadIdx;
static LRA_SIM_PER_LANE SimIdx blockIdx;
static LRA_SIM_PER_LANE SimIdx blockDim;
static LRA_SIM_PER_LANE SimIdx gridDim;

#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(...)
using std::exp;
using std::expm1;
using std::hypot;
using std::log;
using std::log10;
using std::log1p;
using std::pow;
using std::rint;
using std::sqrt;

alignas(16) static unsigned char g_postsim_dyn_lds[160 * 1024];  // the dynamic LDS of the workgroup being run

namespace sim {
constexpr unsigned kWave = 64, kMaxBlock = 1024;

inline void set_lane(unsigned t, unsigned b, unsigned block, unsigned grid) {
    threadIdx.x = t;
    blockIdx.x = b;
    blockDim.x = block;
    gridDim.x = grid;
}

// kernels without __syncthreads: the lanes of a workgroup one after the other on the calling thread (either scheduler)
template <class F> void run_grid_serial(unsigned grid, unsigned block, F body) {
    for (unsigned b = 0; b < grid; ++b)
        for (unsigned t = 0; t < block; ++t) {
            set_lane(t, b, block, grid);
            body();
        }
}

#ifdef LRA_SIM_THREADS
struct Barrier {
    std::mutex m;
    std::condition_variable cv;
    unsigned n = 0, waiting = 0;
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
static Barrier g_block, g_wave[kMaxBlock / kWave];
inline void meet_block() { g_block.wait(); }
inline void meet_wave() { g_wave[threadIdx.x / kWave].wait(); }

template <class F> void run_grid(unsigned grid, unsigned block, F body) {
    g_block.n = block;
    for (unsigned w = 0; w * kWave < block; ++w) g_wave[w].n = block - w * kWave < kWave ? block - w * kWave : kWave;
    for (unsigned b = 0; b < grid; ++b) {
        std::vector<std::thread> lanes;
        for (unsigned t = 0; t < block; ++t)
            lanes.emplace_back([=] {
                set_lane(t, b, block, grid);
                body();
            });
        for (auto& l : lanes) l.join();
    }
}
#else
struct Fibre {
    ucontext_t ctx;
    std::vector<char> stack;
    bool done = false;
};
static ucontext_t g_sched;
static std::vector<Fibre> g_fibres;
static Fibre* g_cur = nullptr;
static std::function<void()> g_body;

inline void fibre_main() {
    g_body();
    g_cur->done = true;
}
inline void meet_block() { swapcontext(&g_cur->ctx, &g_sched); }
inline void meet_wave() { meet_block(); }  // a sweep over the workgroup's fibres is a meeting of each of its waves too

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
        for (bool live = true; live;) {
            live = false;
            for (unsigned t = 0; t < block; ++t) {
                Fibre& f = g_fibres[t];
                if (f.done) continue;
                g_cur = &f;
                set_lane(t, b, block, grid);  // on every resumption: the indices are the running lane's after a hand-over as before it
                swapcontext(&g_sched, &f.ctx);
                live = live || !f.done;
            }
        }
    }
}
#endif

// ---- the wave stand-ins -------------------------------------------------------------------------------------------------------------------
template <class T> T* wave_slots() {
    static T slots[kMaxBlock];
    return slots;
}
// post v, meet, take read(the workgroup's slots, my thread index), meet
template <class T, class F> auto wave_exchange(T v, F read) {
    T* s = wave_slots<T>();
    const unsigned me = threadIdx.x;
    s[me] = v;
    meet_wave();
    const auto r = read((const T*)s, me);
    meet_wave();
    return r;
}
// the value that thread from(me) posted (a lane of my own wave: the waves do not meet each other)
template <class T, class F> T wave_read(T v, F from) {
    return wave_exchange(v, [&](const T* s, unsigned me) { return s[from(me)]; });
}
// op folded over the values of my wave's lanes, in lane order
template <class T, class F> T wave_reduce(T v, F op) {
    return wave_exchange(v, [&](const T* s, unsigned me) {
        const unsigned w0 = me & ~(kWave - 1), lanes = blockDim.x - w0 < kWave ? blockDim.x - w0 : kWave;
        T acc = s[w0];
        for (unsigned l = 1; l < lanes; ++l) acc = op(acc, s[w0 + l]);
        return acc;
    });
}
// bit l: the predicate of lane l of my wave
inline unsigned long long wave_ballot(int pred) {
    return wave_exchange<int>(pred != 0, [](const int* s, unsigned me) {
        const unsigned w0 = me & ~(kWave - 1), lanes = blockDim.x - w0 < kWave ? blockDim.x - w0 : kWave;
        unsigned long long votes = 0;
        for (unsigned l = 0; l < lanes; ++l) votes |= (unsigned long long)(s[w0 + l] != 0) << l;
        return votes;
    });
}
}  // namespace sim

static inline void __syncthreads() { sim::meet_block(); }
using sim::run_grid;
using sim::run_grid_serial;
