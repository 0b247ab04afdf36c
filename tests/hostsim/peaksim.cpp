// peaksim.cpp -- runs the peak-picking kernel bodies of librosa_amd/csrc/lra_peaks.h on host threads (tests/hostsim/simshim.h).
//
// TEST INFRASTRUCTURE ONLY.  Built by tests/hostsim_util.py (sim_lib) into tests/hostsim/_peaksim.so.
// Never linked into, imported by, or used as a fallback for the product library.
// With -DPEAKSIM_MAIN the file is a program of its own (a few fixed rows through every kernel), for a stand-alone sanitizer build.
#define LRA_SIM_THREADS 1
#include "simshim.h"

namespace lra {
namespace peaks {
unsigned long long peaks_wave_ballot(int pred) { return sim::wave_ballot(pred); }
}  // namespace peaks
}  // namespace lra

#include "../../librosa_amd/csrc/lra_peaks.h"

namespace {
template <class T> void run_pick(const lra::peaks::Args& a, long long batch) {
    using namespace lra::peaks;
    run_grid((unsigned)batch, kStatsNT, [=] { peak_stats_kernel<T>(a); });
    run_grid((unsigned)(batch * ((a.n + kTile - 1) / kTile)), kTile, [=] { peak_candidates_kernel<T>(a); });
    if (a.method == kGreedy) run_grid((unsigned)batch, kWave, [=] { peak_greedy_kernel<T>(a); });
    else run_grid((unsigned)batch, kWave, [=] { peak_dp_kernel<T>(a); });
}
}  // namespace

extern "C" {
int peaksim_tile() { return lra::peaks::kTile; }
int peaksim_halo() { return lra::peaks::kHalo; }
int peaksim_ring() { return lra::peaks::kRing; }

// the arguments of lra_peak_pick_exec (include/librosa_amd.h), host pointers; norm ([batch][n] of the rows' type) receives the normalised
// rows, cand ([batch][n]) the candidate flags, status the two bits
int peaksim_pick(const void* x, long long batch, long long n, int is_f64, int normalize, long long pre_max, long long post_max, long long pre_avg, long long post_avg, double delta,
                 long long wait, int method, unsigned char* out, void* norm, unsigned char* cand, int* status) {
    using namespace lra::peaks;
    *status = 2;
    if (batch <= 0 || n <= 0) return 0;
    std::vector<double> values((size_t)batch * (size_t)(n + 1));
    std::vector<unsigned long long> taken((size_t)batch * (size_t)((n + 63) / 64));
    int st[2] = {0, 0};
    Args a{};
    a.x = x;
    a.n = n;
    a.normalize = normalize != 0;
    a.pre_max = (int)clamp_window(pre_max, n);
    a.post_max = (int)clamp_window(post_max, n);
    a.pre_avg = (int)clamp_window(pre_avg, n);
    a.post_avg = (int)clamp_window(post_avg, n);
    a.wait = (int)clamp_window(wait, n);
    a.delta = delta;
    a.method = method;
    a.norm = norm;
    a.cand = cand;
    a.values = values.data();
    a.taken = taken.data();
    a.status = st;
    a.out = out;
    if (is_f64) run_pick<double>(a, batch);
    else run_pick<float>(a, batch);
    *status = (st[0] ? 1 : 0) | (st[1] ? 0 : 2);
    return 0;
}

// lra_prev_minimum_exec, host pointers
int peaksim_prev_minimum(const void* energy, long long batch, long long m, int is_f64, int* out) {
    using namespace lra::peaks;
    if (batch <= 0 || m <= 0) return 0;
    MinArgs a{energy, m, out};
    if (is_f64) run_grid((unsigned)batch, kWave, [=] { prev_minimum_kernel<double>(a); });
    else run_grid((unsigned)batch, kWave, [=] { prev_minimum_kernel<float>(a); });
    return 0;
}
}

#ifdef PEAKSIM_MAIN
int main() {
    int bad = 0;
    for (long long n : {1LL, 2LL, 3LL, 63LL, 64LL, 65LL, 257LL, 700LL, 2200LL})
        for (int method = 0; method < 3; ++method)
            for (long long wide : {0LL, 1LL}) {
                const long long batch = 2;
                std::vector<float> x((size_t)(batch * n)), norm(x.size());
                for (size_t i = 0; i < x.size(); ++i) x[i] = (float)((i * 2654435761u) % 1000u) / 1000.0f;
                std::vector<unsigned char> out(x.size(), 0xFF), cand(x.size(), 0xFF);
                std::vector<int> prev(x.size(), -7);
                int status = 0;
                peaksim_pick(x.data(), batch, n, 0, 1, wide ? 300 : 3, wide ? 1000 : 2, wide ? 70 : 4, 5, 0.05, wide ? 2100 : 3, method, out.data(), norm.data(), cand.data(), &status);
                peaksim_prev_minimum(norm.data(), batch, n, 0, prev.data());
                for (size_t i = 0; i < x.size(); ++i) bad += out[i] > 1 || cand[i] > 1 || prev[i] < 0 || prev[i] > (int)(i % (size_t)n);
            }
    std::printf("peaksim: %d bad entries\n", bad);
    return bad != 0;
}
#endif
