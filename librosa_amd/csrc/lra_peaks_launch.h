// lra_peaks_launch.h -- what lra_api.hip sees of the peak-picking kernels (lra_peaks.h): the launchers, defined in lra_peaks_inst.hip, a
// translation unit of its own.
#pragma once

#include <hip/hip_runtime.h>

#include "lra_peaks.h"

namespace lra {
namespace peaks {
// statistics / normalisation, candidates and the selection of a.method on `batch` rows, in this order on `stream`; f64: the rows' type
hipError_t launch_peak_pick(const Args& a, long long batch, bool f64, hipStream_t stream);
// the preceding-minimum rows of `batch` energy rows
hipError_t launch_prev_minimum(const MinArgs& a, long long batch, bool f64, hipStream_t stream);
}  // namespace peaks
}  // namespace lra
