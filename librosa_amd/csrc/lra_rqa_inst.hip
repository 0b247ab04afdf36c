// lra_rqa_inst.hip -- the RQA kernels (lra_rqa.h) and their launchers and the C entry points they serve, a translation unit of its own so that it
// compiles side by side with lra_api.hip and the other instance groups (librosa_amd/build.py).
#define LRA_RQA_KERNELS 1
#include "lra_rqa.h"

#include "lra_internal.h"

namespace lra {
namespace rqa {

hipError_t launch_score(ScoreArgs a, int rows, int strip, hipStream_t stream) {
    if (a.N <= 0 || a.M <= 0) return hipSuccess;
    if ((rows != 0 && !rows_ok(rows)) || (strip != 0 && !strip_ok(strip))) return hipErrorInvalidValue;
    a.g = geometry(rows, strip);
    const ScoreKernel kern = score_kernel(a.g.iters, a.f64);
    if (!kern || a.g.iters > kMaxIters) return hipErrorInvalidConfiguration;
    const long long grid = (a.M + a.g.strip - 1) / a.g.strip;
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    for (long long row0 = 0; row0 < a.N; row0 += a.g.rows) {
        a.row0 = row0;
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3((unsigned)a.g.nt), a.g.lds, stream, a);
    }
    return hipGetLastError();
}

hipError_t launch_argmax(ArgmaxArgs a, hipStream_t stream) {
    if (a.count <= 0) return hipErrorInvalidValue;
    a.parts = argmax_parts(a.count);
    hipLaunchKernelGGL(rqa_argmax_part, dim3((unsigned)a.parts), dim3(kArgNT), 0, stream, a);
    hipLaunchKernelGGL(rqa_argmax_final, dim3(1), dim3(kArgNT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_backtrack(const BackArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(rqa_backtrack, dim3(1), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rqa
}  // namespace lra

// ---- C entry points: sequence.rqa ----------------------------------------------------------------------------------------------------------------
using namespace lra;

extern "C" {

static_assert(rqa::kF32 == LRA_F32 && rqa::kF64 == LRA_F64, "rqa types");
static_assert(rqa::kWorkBytes == LRA_RQA_WORK_BYTES, "rqa work area");
static_assert(rqa::geometry(64, 1024).iters <= rqa::kMaxIters && rqa::geometry(64, 1024).lds <= 64 * 1024, "rqa: the largest geometry fits");

int64_t lra_rqa_lds_bytes(int rows, int strip) {
    if ((rows != 0 && !rqa::rows_ok(rows)) || (strip != 0 && !rqa::strip_ok(strip))) return 0;
    return rqa::geometry(rows, strip).lds;
}

int lra_rqa_score_exec(lra_ctx* ctx, const void* sim, int dtype, int64_t N, int64_t M, double gap_onset, double gap_extend, int knight_moves, int rows, int strip, void* score,
                       void* pointers) {
    LRA_BIND(ctx);
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "rqa: sim must be LRA_F32 or LRA_F64");
    if (N < 1 || M < 1) return fail(LRA_EINVAL, "rqa: sim is empty");
    if (lra_rqa_lds_bytes(rows, strip) == 0) return fail(LRA_EINVAL, "rqa: rows is 0 (the library's choice) or a power of two up to 64, strip 0 or a power of two from 4 to 1024");
    if (!sim || !score || !pointers) return fail(LRA_EINVAL, "null data pointer");
    rqa::ScoreArgs a{};
    a.sim = sim;
    a.f64 = dtype == LRA_F64;
    a.N = N;
    a.M = M;
    a.gap_onset = gap_onset;
    a.gap_extend = gap_extend;
    a.knight = knight_moves != 0;
    a.score = score;
    a.ptr = (int8_t*)pointers;
    LRA_HIP(rqa::launch_score(a, rows, strip, ctx->stream));
    return LRA_OK;
}

int lra_rqa_argmax_exec(lra_ctx* ctx, const void* score, int dtype, int64_t count, void* work) {
    LRA_BIND(ctx);
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "rqa: score must be LRA_F32 or LRA_F64");
    if (count < 1) return fail(LRA_EINVAL, "rqa: score is empty");
    if (!score || !work) return fail(LRA_EINVAL, "null data pointer");
    rqa::ArgmaxArgs a{};
    a.score = score;
    a.f64 = dtype == LRA_F64;
    a.count = count;
    a.out = (long long*)work;
    a.part_i = (long long*)((char*)work + 16);
    a.part_v = (double*)((char*)work + 16 + 8 * rqa::kMaxParts);
    LRA_HIP(rqa::launch_argmax(a, ctx->stream));
    return LRA_OK;
}

int lra_rqa_backtrack_exec(lra_ctx* ctx, const void* pointers, int64_t N, int64_t M, void* work, void* path, int64_t* length) {
    LRA_BIND(ctx);
    if (N < 1 || M < 1) return fail(LRA_EINVAL, "rqa: the pointer matrix is empty");
    if (!pointers || !work || !path || !length) return fail(LRA_EINVAL, "null data pointer");
    rqa::BackArgs a{};
    a.ptr = (const int8_t*)pointers;
    a.N = N;
    a.M = M;
    a.start = (const long long*)work;
    a.path = (unsigned long long*)path;
    a.cap = N < M ? N : M;
    a.length = (long long*)((char*)work + 8);
    LRA_HIP(rqa::launch_backtrack(a, ctx->stream));
    long long h = 0;
    LRA_TRY(read_status(ctx, (char*)work + 8, &h, sizeof(h)));
    *length = h;
    return LRA_OK;
}

}  // extern "C"
