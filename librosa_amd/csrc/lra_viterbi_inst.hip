// lra_viterbi_inst.hip -- the Viterbi kernels (lra_viterbi.h) and their launchers, a translation unit of its own so that it compiles side by
// side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#define LRA_VITERBI_KERNELS 1
#include "lra_viterbi.h"

#include "lra_viterbi_launch.h"

namespace lra {
namespace viterbi {

hipError_t launch_prep(const PrepArgs& a, hipStream_t stream) {
    if (a.clips <= 0 || a.T <= 0 || a.S <= 0) return hipSuccess;
    const long long grid = a.kind == kBinary ? (a.clips * a.T + kPrepNT - 1) / kPrepNT : a.clips * ((a.T + kPrepSteps - 1) / kPrepSteps);
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    if (a.kind == kBinary) hipLaunchKernelGGL(viterbi_prep_binary, dim3((unsigned)grid), dim3(kPrepNT), 0, stream, a);
    else hipLaunchKernelGGL(viterbi_prep, dim3((unsigned)grid), dim3(kPrepNT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_decode(const Args& a, hipStream_t stream) {
    if (a.chains <= 0 || a.T <= 0) return hipSuccess;
    const Geometry& g = a.g;
    if (g.lds > kLdsMax || g.nt > kWgMaxNT) return hipErrorInvalidConfiguration;
    const long long grid = g.small ? (a.chains + kSmallNT / g.lanes - 1) / (kSmallNT / g.lanes) : a.chains;
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    void (*kern)(Args) = g.small ? viterbi_small : viterbi_wg;
    if (g.lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, g.lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(g.nt), g.lds, stream, a);
    return hipGetLastError();
}

}  // namespace viterbi
}  // namespace lra
