// lra_pyin_inst.hip -- the pYIN observation and finish kernels (lra_pyin.h) and their launchers, a translation unit of its own so that it
// compiles side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#define LRA_PYIN_KERNELS 1
#include "lra_pyin.h"

#include "lra_pyin_launch.h"

namespace lra {
namespace pyin {

hipError_t launch_obs(const ObsArgs& a, hipStream_t stream) {
    if (a.clips <= 0 || a.T <= 0) return hipSuccess;
    const Geometry& g = a.g;
    if (g.lds > kLdsMax || g.waves < 1 || g.waves > kMaxWaves) return hipErrorInvalidConfiguration;
    const long long grid = (a.clips * a.T + g.waves - 1) / g.waves;
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    if (g.lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pyin_obs), hipFuncAttributeMaxDynamicSharedMemorySize, g.lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(pyin_obs, dim3((unsigned)grid), dim3(64 * g.waves), g.lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_finish(const FinishArgs& a, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    const long long grid = (a.n + kFinishNT - 1) / kFinishNT;
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(pyin_finish, dim3((unsigned)grid), dim3(kFinishNT), 0, stream, a);
    return hipGetLastError();
}

}  // namespace pyin
}  // namespace lra
