// beatsim.cpp -- runs the beat-tracker kernel bodies of librosa_amd/csrc/lra_beat.h on host threads (tests/hostsim/simshim.h).
//
// TEST INFRASTRUCTURE ONLY.  Built by tests/hostsim_util.py (sim_lib) into tests/hostsim/_beatsim.so.
// Never linked into, imported by, or used as a fallback for the product library.
#define LRA_SIM_THREADS 1
#include "simshim.h"

namespace lra {
namespace beat {
double beat_wave_max(double v) { return sim::wave_reduce(v, [](double m, double x) { return x > m ? x : m; }); }
long long beat_wave_max_ll(long long v) { return sim::wave_reduce(v, [](long long m, long long x) { return x > m ? x : m; }); }
long long beat_wave_sum_ll(long long v) { return sim::wave_reduce(v, [](long long s, long long x) { return s + x; }); }
unsigned long long beat_wave_ballot(int pred) { return sim::wave_ballot(pred); }
int beat_wave_read(int v, int lane) { return sim::wave_read(v, [=](unsigned me) { return (me & ~63u) + (unsigned)lane; }); }
}  // namespace beat
}  // namespace lra

#include "../../librosa_amd/csrc/lra_beat.h"

namespace {
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
