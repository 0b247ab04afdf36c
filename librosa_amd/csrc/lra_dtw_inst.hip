// lra_dtw_inst.hip -- the DTW kernels (lra_dtw.h) and their launchers, a translation unit of its own so that it compiles side by side with
// lra_api.hip and the other instance groups (librosa_amd/build.py).
#define LRA_DTW_KERNELS 1
#include "lra_dtw.h"

#include "lra_dtw_launch.h"

namespace lra {
namespace dtw {

static bool grid_fits(long long grid) { return grid > 0 && grid <= 0x7fffffffLL; }

hipError_t launch_cost(const CostArgs& a, hipStream_t stream) {
    if (a.N <= 0 || a.M <= 0) return hipSuccess;
    const long long grid = ((a.N + kCostTile - 1) / kCostTile) * ((a.M + kCostTile - 1) / kCostTile);
    if (!grid_fits(grid)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(dtw_cost, dim3((unsigned)grid), dim3(kCostNT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_prepare(const PrepArgs& a, hipStream_t stream) {
    if (a.count <= 0) return hipSuccess;
    const long long grid = (a.count + kPrepNT - 1) / kPrepNT;
    if (!grid_fits(grid)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(dtw_prepare, dim3((unsigned)grid), dim3(kPrepNT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_widen(const WidenArgs& a, hipStream_t stream) {
    if (a.count <= 0) return hipSuccess;
    const long long grid = (a.count + kPrepNT - 1) / kPrepNT;
    if (!grid_fits(grid)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(dtw_widen, dim3((unsigned)grid), dim3(kPrepNT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_accumulate(AccArgs a, int tile, hipStream_t stream) {
    if (a.N <= 0 || a.M <= 0) return hipSuccess;
    if (tile != 0 && !tile_ok(tile)) return hipErrorInvalidValue;
    if (a.st.n < 1 || a.st.n > kMaxSteps || a.st.max0 < 0 || a.st.max0 > kMaxStep || a.st.max1 < 0 || a.st.max1 > kMaxStep) return hipErrorInvalidValue;
    a.g = geometry(tile, a.st.max0, a.st.max1);
    if (a.g.lds > kLdsMax) return hipErrorInvalidConfiguration;
    a.tiles_n = (a.N + a.g.tile - 1) / a.g.tile;
    a.tiles_m = (a.M + a.g.tile - 1) / a.g.tile;
    void (*kern)(AccArgs) = a.st.n == 3 ? dtw_accumulate : dtw_accumulate_any;
    if (a.g.lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, a.g.lds);
        if (e != hipSuccess) return e;
    }
    for (long long diag = 0; diag < a.tiles_n + a.tiles_m - 1; ++diag) {
        const long long grid = diag_tiles(diag, a.tiles_n, a.tiles_m).count;
        if (!grid_fits(grid)) return hipErrorInvalidConfiguration;
        a.diag = diag;
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kAccNT), a.g.lds, stream, a);
    }
    return hipGetLastError();
}

hipError_t launch_backtrack(const BackArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(dtw_backtrack, dim3(1), dim3(kBackNT), 0, stream, a);
    return hipGetLastError();
}

}  // namespace dtw
}  // namespace lra
