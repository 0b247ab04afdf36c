// lra_rhythm_launch.h -- what lra_api.hip sees of the tempogram kernels (lra_rhythm.h): the transform length for a window length and the
// launchers (defined in lra_rhythm_inst.hip, a translation unit of its own).
#pragma once

#include <hip/hip_runtime.h>

#include "lra_mixed_launch.h"
#include "lra_rhythm.h"

namespace lra {
namespace rhythm {
// the smallest size of LRA_MIXED_SIZES that holds the linear autocorrelation of W samples (2 W - 1), or 0: the direct kernel
constexpr int transform_length(int W) {
    int best = 0;
#define LRA_RHYTHM_CASE(N) \
    if (N >= 2 * W - 1 && (best == 0 || N < best)) best = N;
    LRA_MIXED_SIZES(LRA_RHYTHM_CASE)
#undef LRA_RHYTHM_CASE
    return best;
}
hipError_t launch_tempogram(const Args& a, long long batch, hipStream_t stream);
hipError_t launch_tempo_finish(const FinishArgs& a, long long batch, hipStream_t stream);
}  // namespace rhythm
}  // namespace lra
