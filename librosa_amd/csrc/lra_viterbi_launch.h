// lra_viterbi_launch.h -- what lra_api.hip sees of the Viterbi kernels (lra_viterbi.h): the launchers (defined in lra_viterbi_inst.hip, a
// translation unit of its own).
#pragma once

#include <hip/hip_runtime.h>

#include "lra_viterbi.h"

namespace lra {
namespace viterbi {
hipError_t launch_prep(const PrepArgs& a, hipStream_t stream);
hipError_t launch_decode(const Args& a, hipStream_t stream);
}  // namespace viterbi
}  // namespace lra
