// lra_peaks_inst.hip -- instances and the launchers of the peak-picking kernels (lra_peaks.h), a translation unit of its own so that it
// compiles side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#include "lra_peaks.h"

#include "lra_peaks_launch.h"

namespace lra {
namespace peaks {

template <class T> static hipError_t launch_typed(const Args& a, long long batch, hipStream_t stream) {
    const long long tiles = (a.n + kTile - 1) / kTile;
    if (batch > 0x7fffffffLL || tiles * batch > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(peak_stats_kernel<T>, dim3((unsigned)batch), dim3(kStatsNT), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(peak_candidates_kernel<T>, dim3((unsigned)(tiles * batch)), dim3(kTile), 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.method == kGreedy) hipLaunchKernelGGL(peak_greedy_kernel<T>, dim3((unsigned)batch), dim3(kWave), 0, stream, a);
    else hipLaunchKernelGGL(peak_dp_kernel<T>, dim3((unsigned)batch), dim3(kWave), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_peak_pick(const Args& a, long long batch, bool f64, hipStream_t stream) {
    if (batch <= 0 || a.n <= 0) return hipSuccess;
    return f64 ? launch_typed<double>(a, batch, stream) : launch_typed<float>(a, batch, stream);
}

hipError_t launch_prev_minimum(const MinArgs& a, long long batch, bool f64, hipStream_t stream) {
    if (batch <= 0 || a.m <= 0) return hipSuccess;
    if (batch > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    if (f64) hipLaunchKernelGGL(prev_minimum_kernel<double>, dim3((unsigned)batch), dim3(kWave), 0, stream, a);
    else hipLaunchKernelGGL(prev_minimum_kernel<float>, dim3((unsigned)batch), dim3(kWave), 0, stream, a);
    return hipGetLastError();
}

}  // namespace peaks
}  // namespace lra
