// lra_beat_inst.hip -- instances and the launcher of the beat-tracker kernels (lra_beat.h), a translation unit of its own so that it compiles
// side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#include "lra_beat.h"

#include "lra_beat_launch.h"

namespace lra {
namespace beat {

template <class T> static hipError_t launch_typed(const Args& a, long long batch, hipStream_t stream) {
    const long long blocks = (a.n + 255) / 256;
    if (batch > 0x7fffffffLL || blocks * batch > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(beat_prepare_kernel<T>, dim3((unsigned)batch), dim3(kBeatPrepNT), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(beat_local_score_kernel<T>, dim3((unsigned)(blocks * batch)), dim3(256), 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(beat_track_kernel<T>, dim3((unsigned)batch), dim3(kBeatWave), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_beat(const Args& a, long long batch, bool f64, hipStream_t stream) {
    if (batch <= 0 || a.n <= 0) return hipSuccess;
    return f64 ? launch_typed<double>(a, batch, stream) : launch_typed<float>(a, batch, stream);
}

}  // namespace beat
}  // namespace lra
