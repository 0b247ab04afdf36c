// lra_beat_launch.h -- what lra_api.hip sees of the beat-tracker kernels (lra_beat.h): the launchers, defined in lra_beat_inst.hip, a
// translation unit of its own.
#pragma once

#include <hip/hip_runtime.h>

#include "lra_beat.h"

namespace lra {
namespace beat {
// prepare, local score and the tracker on `batch` rows, in this order on `stream`; f64: the envelope's type
hipError_t launch_beat(const Args& a, long long batch, bool f64, hipStream_t stream);
}  // namespace beat
}  // namespace lra
