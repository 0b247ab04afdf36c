// lra_rqa_launch.h -- what lra_api.hip sees of the RQA kernels (lra_rqa.h): the launchers (defined in lra_rqa_inst.hip, a translation unit of
// its own).
#pragma once

#include <hip/hip_runtime.h>

#include "lra_rqa.h"

namespace lra {
namespace rqa {
// every block of rows of the matrix, one launch each, in stream order (a.row0 and a.g are set here); rows, strip: 0 for the library's choice
hipError_t launch_score(ScoreArgs a, int rows, int strip, hipStream_t stream);
// both stages (a.parts is set here)
hipError_t launch_argmax(ArgmaxArgs a, hipStream_t stream);
hipError_t launch_backtrack(const BackArgs& a, hipStream_t stream);
}  // namespace rqa
}  // namespace lra
