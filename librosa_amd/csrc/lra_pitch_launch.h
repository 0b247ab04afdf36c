// lra_pitch_launch.h -- what lra_api.hip sees of the pitch kernels (lra_pitch.h): the launchers, defined in lra_pitch_inst.hip, a
// translation unit of its own.
#pragma once

#include <hip/hip_runtime.h>

#include "lra_pitch.h"

namespace lra {
namespace pitch {
// the tracker on `batch` clips on `stream`: dense results, or (emit) the peaks into per-frame segments; picks the kernel from the strides
// and fills a.tiles_per_clip
hipError_t launch_piptrack(Args a, long long batch, bool emit, bool f64, hipStream_t stream);
// a.state->thr = np.median of the emitted magnitudes, a.state->total their number; a.hist and a.state must be zero on entry
hipError_t launch_median(SelectArgs a, bool f64, hipStream_t stream);
// the histogram of the tuning residuals into a.out (zero on entry)
hipError_t launch_tuning_hist(HistArgs a, bool f64, hipStream_t stream);
}  // namespace pitch
}  // namespace lra
