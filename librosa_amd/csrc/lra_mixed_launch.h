// lra_mixed_launch.h -- what lra_api.hip (and the tempogram and YIN units, for the table sizes) sees of the mixed-radix kernels: the frame lengths they are instantiated for (lra_mixed_sizes.h,
// checked here against what the kernels can factor) and the launchers (defined in lra_mixed_inst.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "lra_mixed.h"
#include "lra_mixed_sizes.h"

namespace lra {
namespace mixed {
#define LRA_MIXED_CHECK(N) static_assert(supported(N), "n_fft = " #N ": n_fft / 2 must factor into 2, 3, 5 and 7");
LRA_MIXED_SIZES(LRA_MIXED_CHECK)
LRA_MIXED_INV_POW2(LRA_MIXED_CHECK)
LRA_MIXED_FWD_POW2(LRA_MIXED_CHECK)
#undef LRA_MIXED_CHECK
int frames_per_group_of(int n_fft, int elem_bytes);
hipError_t launch_f32(int n_fft, int mode, const Args<float>& a, long long batch, hipStream_t stream);
hipError_t launch_f64(int n_fft, int mode, const Args<double>& a, long long batch, hipStream_t stream);
int cqt_frames_per_group_of(int n_fft, int elem_bytes);
hipError_t launch_cqt_f32(int n_fft, const CqtArgs<float>& a, long long batch, hipStream_t stream);
hipError_t launch_cqt_f64(int n_fft, const CqtArgs<double>& a, long long batch, hipStream_t stream);
hipError_t launch_cqt_multi_f32(int n_fft, const CqtMultiArgs<float>& m, hipStream_t stream);
hipError_t launch_cqt_multi_f64(int n_fft, const CqtMultiArgs<double>& m, hipStream_t stream);
hipError_t launch_irfft_f32(int n_fft, const IrArgs<float>& a, long long clips, hipStream_t stream);   // the inverse real transform alone (frames -> HBM), forward geometry
hipError_t launch_irfft_f64(int n_fft, const IrArgs<double>& a, long long clips, hipStream_t stream);
int inv_frames_max_of(int n_fft, int elem_bytes);  // frames (own + halo) the inverse kernel holds per workgroup
hipError_t launch_inv_f32(int n_fft, const InvArgs<float>& a, long long batch, hipStream_t stream);
hipError_t launch_inv_f64(int n_fft, const InvArgs<double>& a, long long batch, hipStream_t stream);
}  // namespace mixed
}  // namespace lra
