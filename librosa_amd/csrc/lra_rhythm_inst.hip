// lra_rhythm_inst.hip -- instances and launchers of the tempogram kernels (lra_rhythm.h), a translation unit of its own so that it compiles
// side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#include "lra_rhythm.h"

#include "lra_rhythm_launch.h"

namespace lra {
namespace rhythm {

hipError_t launch_tempogram(const Args& a, long long batch, hipStream_t stream) {
    const long long grid = batch * a.groups;
    if (grid <= 0) return hipSuccess;
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    const int lds = lds_layout(a.N, a.W, a.mode, a.tile != 0).total;
    if (lds > kRhythmLdsMax) return hipErrorInvalidConfiguration;
    void (*kern)(Args) = nullptr;
    switch (a.N) {
        case 0: kern = tempogram_kernel<0>; break;
#define LRA_RHYTHM_CASE(N) \
    case N: kern = tempogram_kernel<N>; break;
        LRA_MIXED_SIZES(LRA_RHYTHM_CASE)
#undef LRA_RHYTHM_CASE
        default: return hipErrorInvalidValue;
    }
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kRhythmNT), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_tempo_finish(const FinishArgs& a, long long batch, hipStream_t stream) {
    if (batch <= 0) return hipSuccess;
    if (batch > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(tempo_mean_finish_kernel<double>, dim3((unsigned)batch), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rhythm
}  // namespace lra
