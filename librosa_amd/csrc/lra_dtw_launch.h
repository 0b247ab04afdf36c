// lra_dtw_launch.h -- what lra_api.hip sees of the DTW kernels (lra_dtw.h): the launchers (defined in lra_dtw_inst.hip, a translation unit of
// its own).
#pragma once

#include <hip/hip_runtime.h>

#include "lra_dtw.h"

namespace lra {
namespace dtw {
hipError_t launch_cost(const CostArgs& a, hipStream_t stream);
hipError_t launch_prepare(const PrepArgs& a, hipStream_t stream);
hipError_t launch_widen(const WidenArgs& a, hipStream_t stream);
// every tile anti-diagonal of the matrix, one launch each, in stream order (a.diag, a.tiles_n, a.tiles_m and a.g are set here)
hipError_t launch_accumulate(AccArgs a, int tile, hipStream_t stream);
hipError_t launch_backtrack(const BackArgs& a, hipStream_t stream);
}  // namespace dtw
}  // namespace lra
