// lra_chroma_launch.h -- what lra_api.hip sees of the chroma kernels (lra_chroma.h): the launcher, defined in lra_chroma_inst.hip, a
// translation unit of its own.
#pragma once

#include <hip/hip_runtime.h>

#include "lra_chroma.h"

namespace lra {
namespace chroma {
// projection, threshold and normalisation of `batch` clips on `stream`; picks the kernel from the strides and fills a.tiles_per_clip
hipError_t launch_chroma(Args a, long long batch, bool f64, hipStream_t stream);
}  // namespace chroma
}  // namespace lra
