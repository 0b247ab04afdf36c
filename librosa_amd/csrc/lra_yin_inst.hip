// lra_yin_inst.hip -- instances and launcher of the YIN kernels (lra_yin.h), a translation unit of its own so that it compiles side by side
// with lra_api.hip and the other instance groups (librosa_amd/build.py).
#include "lra_yin.h"

#include "lra_yin_launch.h"

namespace lra {
namespace yin {

hipError_t launch_yin(const Args& a, long long batch, hipStream_t stream) {
    const long long grid = batch * a.groups;
    if (grid <= 0) return hipSuccess;
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    const int lds = lds_layout(a.N, a.max_period).total;
    if (lds > kYinLdsMax) return hipErrorInvalidConfiguration;
    void (*kern)(Args) = nullptr;
    switch (a.N) {
        case 0: kern = yin_kernel<0>; break;
#define LRA_YIN_CASE(N) \
    case N: kern = yin_kernel<N>; break;
        LRA_MIXED_SIZES(LRA_YIN_CASE)
#undef LRA_YIN_CASE
        default: return hipErrorInvalidValue;
    }
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kYinNT), lds, stream, a);
    return hipGetLastError();
}

}  // namespace yin
}  // namespace lra
