// lra_chroma_inst.hip -- instances and the launcher of the chroma kernels (lra_chroma.h), a translation unit of its own so that it compiles
// side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#include "lra_chroma.h"

#include "lra_chroma_launch.h"

namespace lra {
namespace chroma {

template <class T> static hipError_t launch_typed(Args a, long long batch, hipStream_t stream) {
    const bool rows = a.bin_stride == 1;  // frame-major rows: lanes along the bins; anything else: lanes along time
    const int per = rows ? kTileF : kColsF;
    a.tiles_per_clip = (a.n_frames + per - 1) / per;
    if (a.tiles_per_clip * batch > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)(a.tiles_per_clip * batch));
    if (rows) hipLaunchKernelGGL(chroma_rows_kernel<T>, grid, dim3(kNT), 0, stream, a);
    else hipLaunchKernelGGL(chroma_cols_kernel<T>, grid, dim3(kNT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_chroma(Args a, long long batch, bool f64, hipStream_t stream) {
    if (batch <= 0 || a.n_frames <= 0 || a.n_chroma <= 0) return hipSuccess;
    return f64 ? launch_typed<double>(a, batch, stream) : launch_typed<float>(a, batch, stream);
}

}  // namespace chroma
}  // namespace lra
