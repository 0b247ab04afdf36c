// lra_enhance.h -- librosa.segment.path_enhance (librosa/segment.py:1167-1329), the lag transforms util.shear / recurrence_to_lag / lag_to_recurrence
// (librosa/util/utils.py:2136-2260, librosa/segment.py:709-891) and feature.stack_memory (librosa/feature/utils.py:134-314), all on the device.
//
//   enhance_conv   All diagonal filters of path_enhance in one launch.  The host flattens the filters into one tap table, grouped per filter, in the
//                  order scipy.ndimage.convolve visits the flipped kernel (row-major, zero weights left out); a tap is an LDS offset and a float64
//                  weight.  A workgroup owns an output tile of rows x cols cells of one channel.  It stages the tile plus its halo (the reach of
//                  the longest filter) in LDS as float64, with scipy's boundary map applied while staging (reflect, constant, nearest, mirror, wrap;
//                  modulo the period, so a matrix smaller than the kernel folds several times).  A thread owns kOwn cells one below the other:
//                  lanes run along the columns, so the 32 lanes of an LDS lane group read 32 consecutive doubles (every bank once, at any offset
//                  and any row pitch; tiles of 16 columns put two rows into a group and get a pitch of 16 mod 32 doubles).  The tap loop is
//                  a scalar read of (offset, weight) and kOwn LDS reads at `own address + offset`, one product and one sum each, every operation
//                  rounded on its own (contraction off: scipy multiplies and adds, it does not fuse) into a float64 accumulator that starts at 0.
//                  float32 input: the sum is rounded to float32 once per filter.  Across filters a register keeps np.maximum's running result
//                  (a NaN propagates); np.clip(x, 0, None) is applied at the end and the cell is stored once.
//   enhance_shear  out[r][c] = P[(r - factor c) mod rows_p][c] (axis 1), or out[r][c] = P[r][(c - factor r) mod cols_p] (axis 0), where P is the
//                  input [rows_in][cols_in] followed by zeros up to the period (recurrence_to_lag's pad) and out may stop before the period
//                  (lag_to_recurrence's slice).  Elements are moved as 1, 2, 4 or 8 bytes: no value is interpreted.
//   enhance_stack  out[b][step d + i][j] = X[b][i][pad(j - step delay)]: stack_memory straight from the unpadded input, np.pad's index map
//                  (constant, edge, reflect, symmetric, wrap) applied to the source index.  Elements move as bytes as well.
// Everything that scales with the matrix is indexed in 64 bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lra {
namespace enhance {

constexpr int kLdsMax = 160 * 1024;  // LRA_ENHANCE_LDS_MAX
constexpr int kOwn = 4;              // cells a thread owns, one below the other
constexpr int kMaxThreads = 1024;
constexpr int kMaxReach = 124;       // LRA_ENHANCE_MAX_REACH: the halo (rows, and columns) that fits kLdsMax next to the smallest tile
constexpr int kReflect = 0, kConstant = 1, kNearest = 2, kMirror = 3, kWrap = 4;   // the LRA_ENHANCE_* boundary modes
constexpr int kPadConstant = 0, kPadEdge = 1, kPadReflect = 2, kPadSymmetric = 3, kPadWrap = 4;   // the LRA_STACK_* pad modes
constexpr int kMoveNT = 256, kShearTile = 32, kStackPer = 8;

struct Tap {   // one non-zero weight of one filter
    int off;   // row offset * pitch + column offset, from the cell's own LDS address
    int pad;
    double w;
};
static_assert(sizeof(Tap) == 16, "tap layout");

struct Geometry {
    int rows, cols;      // the output tile
    int srows, scols;    // the staged region: tile + halo
    int pitch;           // doubles per staged row
    int threads;
    int lds;             // bytes; 0: not served
};

constexpr bool cols_ok(int cols) { return cols == 16 || cols == 32 || cols == 64; }

// The geometry of a tile of rows x cols under a halo of halo_r rows and halo_c columns.  rows 1 .. 256, cols 16, 32 or 64, at most
// kMaxThreads * kOwn cells, and the staged region within kLdsMax; lds == 0 otherwise.
constexpr Geometry geometry_of(int rows, int cols, int halo_r, int halo_c) {
    Geometry g{rows, cols, 0, 0, 0, 0, 0};
    if (rows < 1 || rows > 256 || !cols_ok(cols) || halo_r < 0 || halo_c < 0 || halo_r > 65535 || halo_c > 65535) return g;
    const int groups = (rows + kOwn - 1) / kOwn;
    const int threads = (groups * cols + 63) / 64 * 64;
    if (threads > kMaxThreads) return g;
    g.srows = rows + halo_r;
    g.scols = cols + halo_c;
    g.pitch = g.scols;
    if (cols == 16) g.pitch = (g.scols + 15) / 32 * 32 + 16;   // two rows per lane group: 16 mod 32 doubles apart
    g.threads = threads;
    const long long bytes = 8LL * g.srows * g.pitch;
    g.lds = bytes <= kLdsMax ? (int)bytes : 0;
    return g;
}

// rows == 0 and cols == 0: the library's choice, the first of the list that fits.
constexpr Geometry geometry(int rows, int cols, int halo_r, int halo_c) {
    if (rows != 0 || cols != 0) return geometry_of(rows, cols, halo_r, halo_c);
    constexpr int choice[][2] = {{64, 64}, {32, 64}, {32, 32}, {16, 32}, {16, 16}, {8, 16}, {4, 16}};
    for (const auto& c : choice) {
        const Geometry g = geometry_of(c[0], c[1], halo_r, halo_c);
        if (g.lds) return g;
    }
    return Geometry{0, 0, 0, 0, 0, 0, 0};
}

struct ConvArgs {
    const void* in;   // [channels][h][w] of float or double
    void* out;
    int f64;
    long long channels, h, w;
    long long tiles_r, tiles_c;
    int n_filters;
    int rmin, cmin;   // the smallest row and column offset of any tap
    int mode;
    double cval;
    int clip;
    Geometry g;
};

struct ShearArgs {
    const void* in;
    void* out;
    int esize;
    long long rows_in, cols_in;     // the input
    long long rows_p, cols_p;       // the period of the sheared axis (the other one equals the input's)
    long long rows_out, cols_out;
    long long factor;
    int axis0;                      // 1: rows are sheared along the columns (axis = 0)
    long long tiles_c;
};

struct StackArgs {
    const void* in;
    void* out;
    int esize;
    long long batch, d, t;
    long long n_steps, delay;
    int mode;
    unsigned long long fill;   // the constant's bytes
    long long chunks;          // pieces of kStackPer * kMoveNT columns per row
};

#ifdef LRA_ENHANCE_KERNELS

// floor modulus for a positive period
__device__ __forceinline__ long long fmod_pos(long long p, long long n) {
    long long q = p % n;
    return q < 0 ? q + n : q;
}

// scipy.ndimage's boundary map of index p onto [0, n); -1: outside (constant)
__device__ __forceinline__ long long ext_index(long long p, long long n, int mode) {
    if (p >= 0 && p < n) return p;
    switch (mode) {
        case kReflect: {
            const long long q = fmod_pos(p, 2 * n);
            return q < n ? q : 2 * n - 1 - q;
        }
        case kMirror: {
            if (n == 1) return 0;
            const long long q = fmod_pos(p, 2 * n - 2);
            return q < n ? q : 2 * n - 2 - q;
        }
        case kWrap:
            return fmod_pos(p, n);
        case kNearest:
            return p < 0 ? 0 : n - 1;
        default:
            return -1;
    }
}

template <typename T>
__device__ __forceinline__ void conv_body(const ConvArgs& a, const Tap* __restrict__ taps, const int* __restrict__ starts) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) char lra_enhance_lds[];
    double* lds = reinterpret_cast<double*>(lra_enhance_lds);
    const Geometry g = a.g;
    const long long tile = blockIdx.x;
    const long long ch = tile / (a.tiles_r * a.tiles_c);
    const long long tr = (tile / a.tiles_c) % a.tiles_r, tc = tile % a.tiles_c;
    const long long r0 = tr * g.rows, c0 = tc * g.cols;
    const T* __restrict__ src = static_cast<const T*>(a.in) + ch * a.h * a.w;

    // stage: a wave per row, lanes along the columns
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    for (int r = wave; r < g.srows; r += waves) {
        const long long sr = ext_index(r0 + a.rmin + r, a.h, a.mode);
        for (int c = lane; c < g.scols; c += 64) {
            const long long sc = ext_index(c0 + a.cmin + c, a.w, a.mode);
            lds[r * g.pitch + c] = (sr < 0 || sc < 0) ? a.cval : (double)src[sr * a.w + sc];
        }
    }
    __syncthreads();

    // the thread's cells: column `col`, rows row + 0 .. kOwn - 1 of the tile (clamped into the tile for the reads, masked at the store)
    const int col = threadIdx.x % g.cols, group = threadIdx.x / g.cols;
    int rows_of[kOwn];
    const double* own[kOwn];
#pragma unroll
    for (int k = 0; k < kOwn; ++k) {
        const int r = group * kOwn + k;
        rows_of[k] = r;
        const int rc = r < g.rows ? r : g.rows - 1;
        own[k] = lds + (rc - a.rmin) * g.pitch + (col - a.cmin);
    }

    double best[kOwn];
    for (int f = 0; f < a.n_filters; ++f) {
        double acc[kOwn];
#pragma unroll
        for (int k = 0; k < kOwn; ++k) acc[k] = 0.0;
        const int t1 = starts[f + 1];
#pragma unroll 4
        for (int t = starts[f]; t < t1; ++t) {
            const Tap tp = taps[t];
#pragma unroll
            for (int k = 0; k < kOwn; ++k) {
                const double prod = own[k][tp.off] * tp.w;
                acc[k] = acc[k] + prod;
            }
        }
#pragma unroll
        for (int k = 0; k < kOwn; ++k) {
            const double v = (double)(T)acc[k];   // the filter's response in the input's type
            // np.maximum(running, v): (running >= v || isnan(running)) ? running : v
            best[k] = f == 0 ? v : ((best[k] >= v || best[k] != best[k]) ? best[k] : v);
        }
    }

    T* __restrict__ dst = static_cast<T*>(a.out) + ch * a.h * a.w;
#pragma unroll
    for (int k = 0; k < kOwn; ++k) {
        const long long r = r0 + rows_of[k], c = c0 + col;
        if (rows_of[k] < g.rows && r < a.h && c < a.w) {
            double v = best[k];
            if (a.clip) v = (v >= 0.0 || v != v) ? v : 0.0;   // np.maximum(v, 0)
            dst[r * a.w + c] = (T)v;
        }
    }
}

__global__ void __launch_bounds__(kMaxThreads) enhance_conv_f64(ConvArgs a, const Tap* __restrict__ taps, const int* __restrict__ starts) { conv_body<double>(a, taps, starts); }
__global__ void __launch_bounds__(kMaxThreads) enhance_conv_f32(ConvArgs a, const Tap* __restrict__ taps, const int* __restrict__ starts) { conv_body<float>(a, taps, starts); }

template <typename E>
__device__ __forceinline__ void shear_body(const ShearArgs& a) {
    const E* __restrict__ in = static_cast<const E*>(a.in);
    E* __restrict__ out = static_cast<E*>(a.out);
    const long long tr = blockIdx.x / a.tiles_c, tc = blockIdx.x % a.tiles_c;
    const long long c = tc * kShearTile + (threadIdx.x % kShearTile);
    if (c >= a.cols_out) return;
    for (int k = threadIdx.x / kShearTile; k < kShearTile; k += kMoveNT / kShearTile) {
        const long long r = tr * kShearTile + k;
        if (r >= a.rows_out) break;
        long long sr = r, sc = c;
        if (a.axis0)
            sc = fmod_pos(c - a.factor * r, a.cols_p);
        else
            sr = fmod_pos(r - a.factor * c, a.rows_p);
        out[r * a.cols_out + c] = (sr < a.rows_in && sc < a.cols_in) ? in[sr * a.cols_in + sc] : E(0);
    }
}

__global__ void __launch_bounds__(kMoveNT) enhance_shear(ShearArgs a) {
    switch (a.esize) {
        case 1: shear_body<uint8_t>(a); break;
        case 2: shear_body<uint16_t>(a); break;
        case 4: shear_body<uint32_t>(a); break;
        default: shear_body<uint64_t>(a); break;
    }
}

// np.pad's map of source index s onto [0, t); -1: the constant
__device__ __forceinline__ long long pad_index(long long s, long long t, int mode) {
    if (s >= 0 && s < t) return s;
    switch (mode) {
        case kPadEdge:
            return s < 0 ? 0 : t - 1;
        case kPadReflect: {
            if (t == 1) return 0;
            const long long q = fmod_pos(s, 2 * t - 2);
            return q < t ? q : 2 * t - 2 - q;
        }
        case kPadSymmetric: {
            const long long q = fmod_pos(s, 2 * t);
            return q < t ? q : 2 * t - 1 - q;
        }
        case kPadWrap:
            return fmod_pos(s, t);
        default:
            return -1;
    }
}

template <typename E>
__device__ __forceinline__ void stack_body(const StackArgs& a) {
    const E* __restrict__ in = static_cast<const E*>(a.in);
    E* __restrict__ out = static_cast<E*>(a.out);
    // a workgroup per piece of kStackPer * kMoveNT columns of one output row: the divisions are the workgroup's, not the lane's
    const long long rows = a.d * a.n_steps;
    const long long line = blockIdx.x / a.chunks, chunk = blockIdx.x % a.chunks;   // line = b * rows + row
    const long long b = line / rows, row = line % rows;
    const long long step = row / a.d, i = row % a.d;
#pragma unroll
    for (int k = 0; k < kStackPer; ++k) {
        const long long j = (chunk * kStackPer + k) * kMoveNT + threadIdx.x;
        if (j >= a.t) return;
        const long long s = pad_index(j - step * a.delay, a.t, a.mode);
        out[line * a.t + j] = s < 0 ? (E)a.fill : in[(b * a.d + i) * a.t + s];
    }
}

__global__ void __launch_bounds__(kMoveNT) enhance_stack(StackArgs a) {
    switch (a.esize) {
        case 1: stack_body<uint8_t>(a); break;
        case 2: stack_body<uint16_t>(a); break;
        case 4: stack_body<uint32_t>(a); break;
        default: stack_body<uint64_t>(a); break;
    }
}

#endif  // LRA_ENHANCE_KERNELS

}  // namespace enhance
}  // namespace lra
