// lra_pyin_launch.h -- what lra_api.hip sees of the pYIN kernels (lra_pyin.h): the launchers (defined in lra_pyin_inst.hip, a translation
// unit of its own).
#pragma once

#include <hip/hip_runtime.h>

#include "lra_pyin.h"

namespace lra {
namespace pyin {
hipError_t launch_obs(const ObsArgs& a, hipStream_t stream);
hipError_t launch_finish(const FinishArgs& a, hipStream_t stream);
}  // namespace pyin
}  // namespace lra
