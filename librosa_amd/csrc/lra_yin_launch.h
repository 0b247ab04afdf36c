// lra_yin_launch.h -- what lra_api.hip sees of the YIN kernels (lra_yin.h): the launcher (defined in lra_yin_inst.hip, a translation unit of its own).
#pragma once

#include <hip/hip_runtime.h>

#include "lra_mixed_launch.h"
#include "lra_yin.h"

namespace lra {
namespace yin {
hipError_t launch_yin(const Args& a, long long batch, hipStream_t stream);
}  // namespace yin
}  // namespace lra
