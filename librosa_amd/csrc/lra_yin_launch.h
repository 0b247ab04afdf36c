// lra_yin_launch.h -- what lra_api.hip sees of the YIN kernels (lra_yin.h): the transform length for a frame length and a longest period, and
// the launcher (defined in lra_yin_inst.hip, a translation unit of its own).
#pragma once

#include <hip/hip_runtime.h>

#include "lra_mixed_launch.h"
#include "lra_yin.h"

namespace lra {
namespace yin {
// the smallest size of LRA_MIXED_SIZES that holds the linear autocorrelation of W samples up to lag P (W + P), or 0: the direct kernel
constexpr int transform_length(int W, int P) {
    int best = 0;
#define LRA_YIN_CASE(N) \
    if (N >= W + P && (best == 0 || N < best)) best = N;
    LRA_MIXED_SIZES(LRA_YIN_CASE)
#undef LRA_YIN_CASE
    return best;
}
hipError_t launch_yin(const Args& a, long long batch, hipStream_t stream);
}  // namespace yin
}  // namespace lra
