// onsetsim.cpp -- runs the onset-strength kernel bodies of librosa_amd/csrc/lra_onset.h on host threads (tests/hostsim/simshim.h).
//
// TEST INFRASTRUCTURE ONLY.  Built by tests/hostsim_util.py (sim_lib) into tests/hostsim/_onsetsim.so.
// Never linked into, imported by, or used as a fallback for the product library.
#define LRA_SIM_THREADS 1
#include "simshim.h"

#include "../../librosa_amd/csrc/lra_onset.h"

namespace {
// the launches of onset_run (lra_api.hip): same geometry, same kernel selection
template <class T, bool DB>
int sim_run(lra::OnsetArgs<T> a, int aggregate, int max_ch_bands, int detrend, void* env, void* out) {
    using namespace lra;
    const int rows = (aggregate == kOnsetNone || aggregate == kOnsetRows) ? a.n_bands : a.n_ch;
    a.out = detrend ? (T*)env : (T*)out;
    if (aggregate == kOnsetMedian) {
        const int fb = onset_median_frames(max_ch_bands, sizeof(T));
        if (fb == 0) return -1;
        const unsigned grid = (unsigned)(a.batch * ((a.n_out + fb - 1) / fb));
        run_grid_serial(grid, (unsigned)fb, [=] { onset_median_kernel<T, DB>(a); });
    } else {
        const unsigned grid = (unsigned)(a.batch * ((a.n_out + 255) / 256));
        switch (aggregate) {
            case kOnsetNone: run_grid_serial(grid, 256, [=] { onset_flux_kernel<T, DB, kOnsetNone>(a); }); break;
            case kOnsetMean: run_grid_serial(grid, 256, [=] { onset_flux_kernel<T, DB, kOnsetMean>(a); }); break;
            case kOnsetSum: run_grid_serial(grid, 256, [=] { onset_flux_kernel<T, DB, kOnsetSum>(a); }); break;
            case kOnsetMax: run_grid_serial(grid, 256, [=] { onset_flux_kernel<T, DB, kOnsetMax>(a); }); break;
            case kOnsetMin: run_grid_serial(grid, 256, [=] { onset_flux_kernel<T, DB, kOnsetMin>(a); }); break;
            default: run_grid_serial(grid, 256, [=] { onset_flux_kernel<T, DB, kOnsetRows>(a); }); break;
        }
    }
    if (detrend) {
        const long long n_rows = a.batch * rows;
        const unsigned grid = (unsigned)((n_rows + kOnsetDetrendRows - 1) / kOnsetDetrendRows);
        const T* e = (const T*)env;
        double* o = (double*)out;
        const long long n = a.n_out;
        run_grid(grid, 64, [=] { onset_detrend_kernel<T>(e, o, n_rows, n); });
    }
    return 0;
}

template <class T>
int sim_dispatch(const void* S, const void* ref, void* out, long long batch, int n_bands, long long n_frames, int lag, int max_size, int aggregate, const int* ch_off, const int* ch_band,
                 int n_ch, int max_ch_bands, long long pad, long long n_out, int fuse_db, double amin, double top_db, const void* item_max, int detrend, void* env) {
    lra::OnsetArgs<T> a;
    a.S = (const T*)S;
    a.ref = (const T*)ref;
    a.out = nullptr;
    a.ch_off = ch_off;
    a.ch_band = ch_band;
    a.batch = batch;
    a.n_frames = n_frames;
    a.pad = pad;
    a.n_out = n_out;
    a.n_bands = n_bands;
    a.lag = aggregate == lra::kOnsetRows ? 0 : lag;
    a.max_size = max_size;
    a.n_ch = n_ch;
    a.db = lra::DbArgs<T>{(T)amin, (T)1, nullptr, (const T*)item_max, (T)top_db};
    return fuse_db ? sim_run<T, true>(a, aggregate, max_ch_bands, detrend, env, out) : sim_run<T, false>(a, aggregate, max_ch_bands, detrend, env, out);
}
}  // namespace

extern "C" {
// the arguments of lra_onset_exec (include/librosa_amd.h), host pointers
int onsetsim_exec(const void* S, const void* ref, void* out, long long batch, int n_bands, long long n_frames, int is_f64, int lag, int max_size, int aggregate, const int* ch_off,
                  const int* ch_band, int n_ch, int max_ch_bands, long long pad, long long n_out, int fuse_db, double amin, double top_db, const void* item_max, int detrend, void* env) {
    if (batch <= 0 || n_out <= 0) return 0;
    return is_f64 ? sim_dispatch<double>(S, ref, out, batch, n_bands, n_frames, lag, max_size, aggregate, ch_off, ch_band, n_ch, max_ch_bands, pad, n_out, fuse_db, amin, top_db, item_max,
                                         detrend, env)
                  : sim_dispatch<float>(S, ref, out, batch, n_bands, n_frames, lag, max_size, aggregate, ch_off, ch_band, n_ch, max_ch_bands, pad, n_out, fuse_db, amin, top_db, item_max,
                                        detrend, env);
}
}
