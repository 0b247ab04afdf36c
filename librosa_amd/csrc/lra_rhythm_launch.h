// lra_rhythm_launch.h -- what lra_api.hip sees of the tempogram kernels (lra_rhythm.h): the launchers (defined in lra_rhythm_inst.hip, a translation unit of its own).
#pragma once

#include <hip/hip_runtime.h>

#include "lra_mixed_launch.h"
#include "lra_rhythm.h"

namespace lra {
namespace rhythm {
hipError_t launch_tempogram(const Args& a, long long batch, hipStream_t stream);
hipError_t launch_tempo_finish(const FinishArgs& a, long long batch, hipStream_t stream);
}  // namespace rhythm
}  // namespace lra
