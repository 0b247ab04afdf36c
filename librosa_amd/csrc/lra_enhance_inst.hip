// lra_enhance_inst.hip -- the path-enhancement, shear and memory-stack kernels (lra_enhance.h) and their launchers and the C entry points they serve,
// a translation unit of its own so that it compiles side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#define LRA_ENHANCE_KERNELS 1
#include "lra_enhance.h"

#include "lra_internal.h"

namespace lra {
namespace enhance {

static bool grid_fits(long long grid) { return grid > 0 && grid <= 0x7fffffffLL; }

hipError_t launch_conv(const ConvArgs& a, const Tap* taps, const int* starts, hipStream_t stream) {
    const long long grid = a.channels * a.tiles_r * a.tiles_c;
    if (!grid_fits(grid)) return hipErrorInvalidConfiguration;
    void (*kern)(ConvArgs, const Tap*, const int*) = a.f64 ? enhance_conv_f64 : enhance_conv_f32;
    if (a.g.lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, a.g.lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(a.g.threads), a.g.lds, stream, a, taps, starts);
    return hipGetLastError();
}

hipError_t launch_shear(ShearArgs a, hipStream_t stream) {
    a.tiles_c = (a.cols_out + kShearTile - 1) / kShearTile;
    const long long grid = a.tiles_c * ((a.rows_out + kShearTile - 1) / kShearTile);
    if (!grid_fits(grid)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(enhance_shear, dim3((unsigned)grid), dim3(kMoveNT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_stack(StackArgs a, hipStream_t stream) {
    a.chunks = (a.t + kStackPer * kMoveNT - 1) / (kStackPer * kMoveNT);
    const long long grid = a.batch * a.d * a.n_steps * a.chunks;
    if (!grid_fits(grid)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(enhance_stack, dim3((unsigned)grid), dim3(kMoveNT), 0, stream, a);
    return hipGetLastError();
}

}  // namespace enhance
}  // namespace lra

// ---- C entry points: segment.path_enhance, util.shear and the lag transforms, feature.stack_memory -------------------------------------------------
using namespace lra;

extern "C" {

static_assert(enhance::kLdsMax == LRA_ENHANCE_LDS_MAX && enhance::kMaxReach == LRA_ENHANCE_MAX_REACH, "enhance limits");
static_assert(enhance::kReflect == LRA_ENHANCE_REFLECT && enhance::kConstant == LRA_ENHANCE_CONSTANT && enhance::kNearest == LRA_ENHANCE_NEAREST && enhance::kMirror == LRA_ENHANCE_MIRROR &&
                  enhance::kWrap == LRA_ENHANCE_WRAP,
              "enhance boundary modes");
static_assert(enhance::kPadConstant == LRA_STACK_CONSTANT && enhance::kPadEdge == LRA_STACK_EDGE && enhance::kPadReflect == LRA_STACK_REFLECT && enhance::kPadSymmetric == LRA_STACK_SYMMETRIC &&
                  enhance::kPadWrap == LRA_STACK_WRAP,
              "stack pad modes");
static_assert(sizeof(lra_enhance_tap) == 16 && sizeof(enhance::Tap) == 16, "tap layout");
static_assert(enhance::geometry(0, 0, enhance::kMaxReach, enhance::kMaxReach).lds > 0, "enhance: the longest reach is served");
static_assert(enhance::geometry(0, 0, 64, 64).rows == 64 && enhance::geometry(0, 0, 64, 64).cols == 64, "enhance: the documented call (n = 51, seven filters, ratio 2) runs at the first choice");

int64_t lra_enhance_lds_bytes(int rows, int cols, int halo_rows, int halo_cols) { return enhance::geometry(rows, cols, halo_rows, halo_cols).lds; }

int lra_path_enhance_exec(lra_ctx* ctx, const void* R, int dtype, int64_t channels, int64_t h, int64_t w, const lra_enhance_tap* taps, const int32_t* starts, int n_filters, int mode,
                          double cval, int clip, int rows, int cols, void* table, void* out) {
    LRA_BIND(ctx);
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "path_enhance: the matrix must be LRA_F32 or LRA_F64");
    if (channels < 1 || h < 1 || w < 1) return fail(LRA_EINVAL, "path_enhance: the matrix is empty");
    if (mode < LRA_ENHANCE_REFLECT || mode > LRA_ENHANCE_WRAP) return fail(LRA_EINVAL, "path_enhance: unknown boundary mode");
    if (n_filters < 1 || !starts) return fail(LRA_EINVAL, "path_enhance: need at least one filter and its taps");
    if (!R || !table || !out) return fail(LRA_EINVAL, "null data pointer");
    if (starts[0] != 0) return fail(LRA_EINVAL, "path_enhance: the first filter's taps start at 0");
    for (int f = 0; f < n_filters; ++f)
        if (starts[f + 1] < starts[f]) return fail(LRA_EINVAL, "path_enhance: the filters' tap ranges must ascend");
    const int n_taps = starts[n_filters];
    if (n_taps > 0 && !taps) return fail(LRA_EINVAL, "path_enhance: need at least one filter and its taps");
    // the reach of the filters: every tap of every filter lies in [rmin, rmax] x [cmin, cmax], and the halo a tile stages is that box
    int rmin = 0, rmax = 0, cmin = 0, cmax = 0;
    for (int t = 0; t < n_taps; ++t) {
        if (taps[t].dr < -LRA_ENHANCE_MAX_REACH || taps[t].dr > LRA_ENHANCE_MAX_REACH || taps[t].dc < -LRA_ENHANCE_MAX_REACH || taps[t].dc > LRA_ENHANCE_MAX_REACH)
            return fail(LRA_EINVAL, "path_enhance: a tap lies more than LRA_ENHANCE_MAX_REACH = " + std::to_string(LRA_ENHANCE_MAX_REACH) + " cells from its output");
        rmin = taps[t].dr < rmin ? taps[t].dr : rmin;
        rmax = taps[t].dr > rmax ? taps[t].dr : rmax;
        cmin = taps[t].dc < cmin ? taps[t].dc : cmin;
        cmax = taps[t].dc > cmax ? taps[t].dc : cmax;
    }
    if (rmax - rmin > LRA_ENHANCE_MAX_REACH || cmax - cmin > LRA_ENHANCE_MAX_REACH)
        return fail(LRA_EINVAL, "path_enhance: the filters reach over more than LRA_ENHANCE_MAX_REACH = " + std::to_string(LRA_ENHANCE_MAX_REACH) + " rows or columns");
    const enhance::Geometry g = enhance::geometry(rows, cols, rmax - rmin, cmax - cmin);
    if (g.lds == 0)
        return fail(LRA_EINVAL, "path_enhance: rows is 0 (the library's choice, with cols 0) or 1 .. 256, cols 16, 32 or 64, rows * cols at most 4096, and the tile and its halo must fit "
                                "LRA_ENHANCE_LDS_MAX = " + std::to_string(LRA_ENHANCE_LDS_MAX) + " bytes of LDS");

    // the device table: the filters' tap ranges, then the taps as (LDS offset, weight)
    const size_t head = LRA_ENHANCE_TABLE_BYTES(0, n_filters);
    std::vector<char> host(LRA_ENHANCE_TABLE_BYTES(n_taps, n_filters));
    int* h_starts = reinterpret_cast<int*>(host.data());
    enhance::Tap* h_taps = reinterpret_cast<enhance::Tap*>(host.data() + head);
    for (int f = 0; f <= n_filters; ++f) h_starts[f] = starts[f];
    for (int t = 0; t < n_taps; ++t) h_taps[t] = enhance::Tap{taps[t].dr * g.pitch + taps[t].dc, 0, taps[t].w};
    LRA_HIP(hipMemcpyAsync(table, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream));
    LRA_HIP(hipStreamSynchronize(ctx->stream));   // (the table lives on this frame)

    enhance::ConvArgs a{};
    a.in = R;
    a.out = out;
    a.f64 = dtype == LRA_F64;
    a.channels = channels;
    a.h = h;
    a.w = w;
    a.tiles_r = (h + g.rows - 1) / g.rows;
    a.tiles_c = (w + g.cols - 1) / g.cols;
    a.n_filters = n_filters;
    a.rmin = rmin;
    a.cmin = cmin;
    a.mode = mode;
    a.cval = cval;
    a.clip = clip != 0;
    a.g = g;
    LRA_HIP(enhance::launch_conv(a, reinterpret_cast<const enhance::Tap*>(static_cast<const char*>(table) + head), static_cast<const int*>(table), ctx->stream));
    return LRA_OK;
}

static bool esize_ok(int esize) { return esize == 1 || esize == 2 || esize == 4 || esize == 8; }

int lra_shear_exec(lra_ctx* ctx, const void* in, int esize, int64_t rows_in, int64_t cols_in, int64_t period, int64_t rows_out, int64_t cols_out, int64_t factor, int axis, void* out) {
    LRA_BIND(ctx);
    if (!esize_ok(esize)) return fail(LRA_EINVAL, "shear: elements of 1, 2, 4 or 8 bytes");
    if (axis != 0 && axis != 1) return fail(LRA_EINVAL, "shear: axis is 0 or 1");
    if (rows_in < 0 || cols_in < 0 || rows_out < 0 || cols_out < 0) return fail(LRA_EINVAL, "shear: negative shape");
    if (rows_out == 0 || cols_out == 0) return LRA_OK;
    // the output lies inside the padded input: the sheared axis within its period, the other within the input
    const int64_t sheared_in = axis == 1 ? rows_in : cols_in, sheared_out = axis == 1 ? rows_out : cols_out;
    const int64_t other_in = axis == 1 ? cols_in : rows_in, other_out = axis == 1 ? cols_out : rows_out;
    if (period < 1 || period < sheared_in || sheared_out > period || other_out > other_in) return fail(LRA_EINVAL, "shear: the output does not lie inside the padded input");
    if (!in || !out) return fail(LRA_EINVAL, "null data pointer");
    enhance::ShearArgs a{};
    a.in = in;
    a.out = out;
    a.esize = esize;
    a.rows_in = rows_in;
    a.cols_in = cols_in;
    a.rows_p = axis == 1 ? period : rows_in;
    a.cols_p = axis == 1 ? cols_in : period;
    a.rows_out = rows_out;
    a.cols_out = cols_out;
    a.factor = factor;
    a.axis0 = axis == 0;
    LRA_HIP(enhance::launch_shear(a, ctx->stream));
    return LRA_OK;
}

int lra_stack_memory_exec(lra_ctx* ctx, const void* in, int esize, int64_t batch, int64_t d, int64_t t, int64_t n_steps, int64_t delay, int mode, uint64_t fill, void* out) {
    LRA_BIND(ctx);
    if (!esize_ok(esize)) return fail(LRA_EINVAL, "stack_memory: elements of 1, 2, 4 or 8 bytes");
    if (mode < LRA_STACK_CONSTANT || mode > LRA_STACK_WRAP) return fail(LRA_EINVAL, "stack_memory: unknown pad mode");
    if (n_steps < 1 || delay == 0 || t < 1 || batch < 0 || d < 0) return fail(LRA_EINVAL, "stack_memory: n_steps >= 1, delay != 0 and at least one column");
    if (batch == 0 || d == 0) return LRA_OK;
    if (!in || !out) return fail(LRA_EINVAL, "null data pointer");
    LRA_HIP(enhance::launch_stack(enhance::StackArgs{in, out, esize, batch, d, t, n_steps, delay, mode, fill, 0}, ctx->stream));
    return LRA_OK;
}

}  // extern "C"
