// lra_pitch_inst.hip -- instances and the launchers of the pitch kernels (lra_pitch.h), a translation unit of its own so that it compiles
// side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#include "lra_pitch.h"

#include "lra_pitch_launch.h"

namespace lra {
namespace pitch {

static unsigned stride_grid(long long n_segments) {
    const long long want = (n_segments + kWaves - 1) / kWaves;
    return (unsigned)(want < 1 ? 1 : (want > kMaxGrid ? kMaxGrid : want));
}

template <class T, bool kEmit> static hipError_t launch_typed(Args a, long long batch, hipStream_t stream) {
    const bool rows = a.bin_stride == 1 && (kEmit || a.out_bin_stride == 1);  // frame-major rows: lanes along the bins; anything else: lanes along time
    const int per = rows ? kRowsF : kColsF;
    a.tiles_per_clip = (a.n_frames + per - 1) / per;
    if (a.tiles_per_clip * batch > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)(a.tiles_per_clip * batch));
    if (rows) hipLaunchKernelGGL((piptrack_rows_kernel<T, kEmit>), grid, dim3(kNT), 0, stream, a);
    else hipLaunchKernelGGL((piptrack_cols_kernel<T, kEmit>), grid, dim3(kNT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_piptrack(Args a, long long batch, bool emit, bool f64, hipStream_t stream) {
    if (batch <= 0 || a.n_frames <= 0 || a.n_bins <= 0) return hipSuccess;
    if (emit) return f64 ? launch_typed<double, true>(a, batch, stream) : launch_typed<float, true>(a, batch, stream);
    return f64 ? launch_typed<double, false>(a, batch, stream) : launch_typed<float, false>(a, batch, stream);
}

template <class T> static hipError_t median_typed(SelectArgs a, hipStream_t stream) {
    const dim3 grid(stride_grid(a.n_segments));
    for (int pass = 0; pass < Passes<T>::value; ++pass) {
        hipLaunchKernelGGL(select_count_kernel<T>, grid, dim3(kNT), 0, stream, a, pass);
        hipLaunchKernelGGL(select_scan_kernel<T>, dim3(1), dim3(kNT), 0, stream, a, pass);
    }
    return hipGetLastError();
}

hipError_t launch_median(SelectArgs a, bool f64, hipStream_t stream) { return f64 ? median_typed<double>(a, stream) : median_typed<float>(a, stream); }

hipError_t launch_tuning_hist(HistArgs a, bool f64, hipStream_t stream) {
    if (a.n_segments <= 0) return hipSuccess;
    const dim3 grid(stride_grid(a.n_segments));
    if (f64) hipLaunchKernelGGL(tuning_hist_kernel<double>, grid, dim3(kNT), 0, stream, a);
    else hipLaunchKernelGGL(tuning_hist_kernel<float>, grid, dim3(kNT), 0, stream, a);
    return hipGetLastError();
}

}  // namespace pitch
}  // namespace lra
