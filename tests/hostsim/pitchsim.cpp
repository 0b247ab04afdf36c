// pitchsim.cpp -- runs the pitch kernel bodies of librosa_amd/csrc/lra_pitch.h on host fibres (tests/hostsim/simshim.h); the atomic adds
// are plain adds.
//
// TEST INFRASTRUCTURE ONLY.  Built by tests/hostsim_util.py (sim_lib) into tests/hostsim/_pitchsim.so.
// Never linked into, imported by, or used as a fallback for the product library.
#define LRA_SIM_FIBRES 1
#include "simshim.h"

namespace lra {
namespace pitch {
double pitch_shfl_xor(double v, int offset) { return sim::wave_read(v, [=](unsigned me) { return me ^ (unsigned)offset; }); }
unsigned long long pitch_ballot(int predicate) { return sim::wave_ballot(predicate); }
}  // namespace pitch
}  // namespace lra

#include "../../librosa_amd/csrc/lra_pitch.h"

namespace {
using namespace lra::pitch;

unsigned stride_grid(long long n_segments) {
    const long long want = (n_segments + kWaves - 1) / kWaves;
    return (unsigned)(want < 1 ? 1 : (want > kMaxGrid ? kMaxGrid : want));
}

void run_piptrack(Args a, long long batch, bool emit, bool f64) {
    const bool rows = a.bin_stride == 1 && (emit || a.out_bin_stride == 1);
    const int per = rows ? kRowsF : kColsF;
    a.tiles_per_clip = (a.n_frames + per - 1) / per;
    const unsigned grid = (unsigned)(a.tiles_per_clip * batch);
    if (rows) {
        if (emit) {
            if (f64) run_grid(grid, kNT, [=] { piptrack_rows_kernel<double, true>(a); });
            else run_grid(grid, kNT, [=] { piptrack_rows_kernel<float, true>(a); });
        } else {
            if (f64) run_grid(grid, kNT, [=] { piptrack_rows_kernel<double, false>(a); });
            else run_grid(grid, kNT, [=] { piptrack_rows_kernel<float, false>(a); });
        }
    } else {
        if (emit) {
            if (f64) run_grid(grid, kNT, [=] { piptrack_cols_kernel<double, true>(a); });
            else run_grid(grid, kNT, [=] { piptrack_cols_kernel<float, true>(a); });
        } else {
            if (f64) run_grid(grid, kNT, [=] { piptrack_cols_kernel<double, false>(a); });
            else run_grid(grid, kNT, [=] { piptrack_cols_kernel<float, false>(a); });
        }
    }
}

template <class T> void run_median(SelectArgs a, unsigned grid) {
    for (int pass = 0; pass < Passes<T>::value; ++pass) {
        run_grid(grid, kNT, [=] { select_count_kernel<T>(a, pass); });
        run_grid(1, kNT, [=] { select_scan_kernel<T>(a, pass); });
    }
}

void run_hist(HistArgs a, bool f64, unsigned grid) {
    if (a.n_segments <= 0) return;
    if (f64) run_grid(grid, kNT, [=] { tuning_hist_kernel<double>(a); });
    else run_grid(grid, kNT, [=] { tuning_hist_kernel<float>(a); });
}

Args make_args(const void* s, long long n_bins, long long n_frames, long long batch_stride, long long bin_stride, long long frame_stride, long long lo, long long hi, int ref_mode,
               double threshold, const double* ref_row, double ref_scalar, double sr, long long n_fft) {
    Args a{};
    a.s = s;
    a.batch_stride = batch_stride;
    a.bin_stride = bin_stride;
    a.frame_stride = frame_stride;
    a.n_bins = (int)n_bins;
    a.n_frames = n_frames;
    a.lo = (int)lo;
    a.hi = (int)hi;
    a.ref_mode = ref_mode;
    a.threshold = threshold;
    a.ref_row = ref_row;
    a.ref_scalar = ref_scalar;
    a.sr = sr;
    a.n_fft = (double)n_fft;
    return a;
}
}  // namespace

extern "C" {
// which: 0 kTile, 1 kRowsF, 2 kColsF, 3 kDigitBits, 4 kHistLds, 5 kPlainSeg, 6 kMaxGrid
int pitchsim_const(int which) {
    const int v[] = {kTile, kRowsF, kColsF, kDigitBits, kHistLds, kPlainSeg, kMaxGrid};
    return v[which];
}

// np.histogram's bin of x among edges[0 .. n] (the last bin closed), -1 outside
int pitchsim_hist_bin(const double* edges, int n, double x) { return hist_bin(edges, n, x); }

// the arguments of lra_piptrack_exec (include/librosa_amd.h), host pointers
int pitchsim_piptrack(const void* s, long long batch, long long n_bins, long long n_frames, long long batch_stride, long long bin_stride, long long frame_stride, int is_f64, long long lo,
                      long long hi, int ref_mode, double threshold, const double* ref_row, double ref_scalar, double sr, long long n_fft, void* pitches, void* mags,
                      long long out_batch_stride, long long out_bin_stride, long long out_frame_stride) {
    if (batch <= 0 || n_frames <= 0 || n_bins <= 0) return 0;
    Args a = make_args(s, n_bins, n_frames, batch_stride, bin_stride, frame_stride, lo, hi, ref_mode, threshold, ref_row, ref_scalar, sr, n_fft);
    a.pitches = pitches;
    a.mags = mags;
    a.out_batch_stride = out_batch_stride;
    a.out_bin_stride = out_bin_stride;
    a.out_frame_stride = out_frame_stride;
    run_piptrack(a, batch, false, is_f64 != 0);
    return 0;
}

// the median of the first count[i] entries of every segment of mag [n_segments][cap]; grid: workgroups of the counting kernel (0: the launcher's choice)
int pitchsim_median(const void* mag, const int* count, long long n_segments, int cap, int is_f64, int grid, void* thr, unsigned long long* total) {
    std::vector<unsigned long long> hist(2 * kDigits, 0ull);
    SelectState st{};
    SelectArgs a{mag, count, n_segments, cap, hist.data(), &st};
    const unsigned g = grid > 0 ? (unsigned)grid : stride_grid(n_segments);
    if (is_f64) run_median<double>(a, g);
    else run_median<float>(a, g);
    std::memcpy(thr, &st.thr, is_f64 ? 8 : 4);
    *total = st.total;
    for (unsigned long long h : hist)
        if (h) return 1;  // the scan leaves the histogram clear
    return 0;
}

// what lra_tuning_exec does: the emitting tracker, the median, the histogram.  peak_pitch / peak_mag [batch * n_frames][cap] and peak_count
// [batch * n_frames] are the caller's (cap = ceil(max(hi - lo, 1) / 2)); out: [n_hist + 2] counts, frequencies counted, peaks; thr: the median as T
int pitchsim_tuning(const void* s, long long batch, long long n_bins, long long n_frames, long long batch_stride, long long bin_stride, long long frame_stride, int is_f64, long long lo,
                    long long hi, int ref_mode, double threshold, const double* ref_row, double ref_scalar, double sr, long long n_fft, const double* edges, long long n_hist,
                    double bins_per_octave, void* peak_pitch, void* peak_mag, int* peak_count, int cap, unsigned long long* out, void* thr) {
    for (long long i = 0; i < n_hist + 2; ++i) out[i] = 0ull;
    const long long n_segments = batch * n_frames;
    Args a = make_args(s, n_bins, n_frames, batch_stride, bin_stride, frame_stride, lo, hi, ref_mode, threshold, ref_row, ref_scalar, sr, n_fft);
    a.peak_pitch = peak_pitch;
    a.peak_mag = peak_mag;
    a.peak_count = peak_count;
    a.cap = cap;
    if (batch > 0 && n_frames > 0 && n_bins > 0) run_piptrack(a, batch, true, is_f64 != 0);
    std::vector<unsigned long long> hist(2 * kDigits, 0ull);
    SelectState st{};
    SelectArgs sa{peak_mag, peak_count, n_segments, cap, hist.data(), &st};
    if (is_f64) run_median<double>(sa, stride_grid(n_segments));
    else run_median<float>(sa, stride_grid(n_segments));
    HistArgs h{peak_pitch, peak_mag, peak_count, n_segments, n_segments * cap, cap, &st, edges, (int)n_hist, bins_per_octave, out};
    run_hist(h, is_f64 != 0, stride_grid(n_segments));
    out[n_hist + 1] = st.total;
    std::memcpy(thr, &st.thr, is_f64 ? 8 : 4);
    return 0;
}

// what lra_pitch_tuning_exec does: the histogram of a plain frequency array
int pitchsim_pitch_tuning(const void* freq, long long n, int is_f64, const double* edges, long long n_hist, double bins_per_octave, unsigned long long* out) {
    for (long long i = 0; i < n_hist + 2; ++i) out[i] = 0ull;
    const long long n_segments = (n + kPlainSeg - 1) / kPlainSeg;
    HistArgs h{freq, nullptr, nullptr, n_segments, n, kPlainSeg, nullptr, edges, (int)n_hist, bins_per_octave, out};
    run_hist(h, is_f64 != 0, stride_grid(n_segments));
    return 0;
}
}
