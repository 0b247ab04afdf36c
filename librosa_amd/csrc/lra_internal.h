// lra_internal.h -- host-side plumbing shared by the translation units that define C entry points: lra_api.hip and the lra_<feature>_inst.hip
// units.  No kernels here.  The context, the error slot and its macros, device binding, and the small allocation helpers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/librosa_amd.h"

namespace lra {

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
// Stores `msg` in the calling thread's error slot (what lra_last_error() returns) and returns `code`.  The slot has one definition, in lra_api.hip:
// a copy per translation unit would leave lra_last_error() blind to every message raised outside the API unit.
int fail(int code, const std::string& msg);

}  // namespace lra

#define LRA_HIP(expr)                                                                                        \
    do {                                                                                                     \
        hipError_t e__ = (expr);                                                                             \
        if (e__ != hipSuccess) return lra::fail(LRA_EHIP, std::string(#expr) + ": " + hipGetErrorString(e__));    \
    } while (0)
#define LRA_FFT(expr)                                                                                        \
    do {                                                                                                     \
        rocfft_status s__ = (expr);                                                                          \
        if (s__ != rocfft_status_success) return lra::fail(LRA_EROCFFT, std::string(#expr) + ": rocfft status " + std::to_string((int)s__)); \
    } while (0)
#define LRA_TRY(expr)              \
    do {                           \
        int rc__ = (expr);         \
        if (rc__ != LRA_OK) return rc__; \
    } while (0)
// (LRA_FFT is for units that include <rocfft/rocfft.h>)

// ------------------------------------------------------------------------------------------------
// objects
// ------------------------------------------------------------------------------------------------
struct lra_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    int n_cu = 256;
    int opt_stft_iters = 0;          // 0 = auto  // [ctx:defaults]
    int opt_istft_strip_groups = 0;  // 0 = auto
    int opt_variant = -1;            // kernel tuning variant (f32 n_fft = 2048 only); -1 = per-mode default
    int opt_autotune = 1;            // variant -1: time the candidate variants on the first large call of a plan and keep the faster
    int opt_mel_runs = 1;            // use the run-ordered two-slope epilogue (OUT_MELR) where it applies
    int opt_mel_tile = 0;            // frames staged per mel row before a flush (0 = auto)
    int opt_generic_mel = 0;         // force the generic banded mel path (tests)
    int opt_lds_pad = 0;             // extra dynamic LDS per workgroup (occupancy experiments)
    int opt_v2 = 1;                  // second-generation forward kernel where it applies (lra_kernels2.h)
    int opt_istft16 = 0;             // inverse, n_fft = 2048 f32, hop = n_fft / {2, 4, 8, 16}: radices 4, 16, 16 with 16-byte spectrum loads (variant 7) instead of 8, 8, 16
    int opt_placement_retry = 0;     // lra_malloc_placed: candidate allocations to time before keeping the best (0 = its `tries` argument decides)
    struct PlacedAlloc {             // one lra_malloc_placed result: a reserved virtual range backed by physical handles created and mapped in order
        size_t padded = 0;
        std::vector<hipMemGenericAllocationHandle_t> handles;
        bool plain = false;          // an ordinary hipMalloc block (candidates of both kinds compete: which kind lands better differs from box to box)
    };
    std::map<void*, PlacedAlloc> placed;
    std::mutex placed_mu;            // lra_free_placed may arrive from a finaliser thread while another call allocates
    // ROCm 7.0 / gfx950, measured (scripts/vmm_coherence.hip, profiles/r06_experiments.md 3): hipMemAddressFree of one reserved range -- or mapping new physical
    // memory into a range that was mapped before -- leaves OTHER live ranges with stale translations (kernels and hipMemcpy read old data: silent corruption).
    // Ranges that are reserved once, never re-used and never freed while anything of this context is alive are clean under any amount of churn.  So: every
    // candidate gets a fresh reservation, a released buffer keeps its (now empty) range until lra_ctx_destroy, and the address space spent that way is budgeted.
    std::vector<std::pair<void*, size_t>> placed_retired;   // reserved ranges whose physical memory is gone: freed at lra_ctx_destroy
    size_t placed_va_spent = 0;
    static constexpr size_t kPlacedVaBudget = (size_t)4 << 40;  // 4 TiB of address space per context, then lra_malloc_placed declines (callers fall back to an ordinary allocation)
    double placed_best_gbps = 0.0;   // best write-stream rate any candidate of this context has shown (the early-exit yardstick)
    int opt_v3 = 1;                  // n_fft = 2048 f32: the radix 16-16-4 form with 16-byte row pieces (variant 6, lra_kernels2.h third form); 1: complex epilogue, 2: |X|^p too
                                     // (measured on two boxes, same buffer, alternating (profiles/r06_raw/c_*, d_*): complex STFT -1.3 % ... -2.0 %, |X|^2 +1 %, hence complex only)
    int opt_mel_pc = 1;              // fused mel, n_fft = 2048 f32: the producer / consumer kernel (lra_kernels_pc.h) instead of stft2_kernel<OUT_MELR>
                                     // (-0.8 ... -1.9 % against the one-wave kernel on four boxes (profiles/r06_raw), never slower)
    int opt_mel_many = 1;            // mel plans of n_fft = 512 with more than 64 bands are built for the eight-bands-per-thread kernel shape (read at lra_mel_plan_create)
    int opt_cqt_merge = 1;           // lra_cqt_recursion_exec: 1 = octaves 1-2 in one launch beside the later halvings, 3 .. in one launch behind the chain (round 6); 2 = octaves 1 .. in one launch per frame length behind the chain (round 5); 0 = one launch per octave on the side stream
    int opt_hpss_tile = 1;           // hpss: a thread per 4 x 4 tile with shared sorted cores (hpss_tile_kernel); 0: a thread per element (A/B)
    int opt_mixed_inv_pow2 = 1;      // inverse, n_fft = 256 / 512 / 1024 with a hop outside n_fft / {2, 4, 8, 16}: the fused gather kernel of lra_mixed.h (0: istft_kernel's general mode)
    int opt_mixed_pow2_mel = 1;      // fused mel at n_fft 128 / 256: the flat-index kernel of lra_mixed.h instead of the register-tiled one (0: A/B)
    int opt_ola4 = 1;                // general inverse path: four output samples per thread in the gather kernel (0: one, A/B)
    int opt_mixed_irfft = 1;         // listed mixed-radix lengths too long for the fused gather kernel: mixed_irfft_kernel + ola_gather_kernel instead of spec_pack + rocFFT + ola_gather (0: A/B)
    int opt_mixed = 1;               // fused mixed-radix forward kernel for the listed non-power-of-two frame lengths (lra_mixed.h); 0: rocFFT path; 2: fused, mel band table read through the caches instead of staged in LDS (A/B)
    int opt_direct = 1;              // direct framing (no ring) for hop >= n_fft
    int opt_xcd_remap = 1;           // workgroup -> work item map that keeps neighbouring strips on one XCD (lra_kernels.h, xcd_block)
    unsigned int* d_flag = nullptr;  // non-finite input flag (device)
    std::map<std::pair<int, int>, std::pair<void*, void*>> cqt_tw;  // (n_fft, dtype) -> (W_M^t, W_N^k) of the fused constant-Q octave kernel (lra_mixed.h)
    std::string name;
    struct HostPipe* pipe = nullptr;  // staging of the host-buffer entry points (lra_stft_exec_host), created on first use
    hipStream_t side_stream = nullptr;  // lra_ctx_side: a second stream for work that may overlap the main chain (created on first fork)
    hipStream_t side_main = nullptr;    // the stream to return to
    // fork: an event recorded on the main stream, waited for by the side stream; join: recorded on the side stream, waited for by the main one.
    // Every fork takes the NEXT event of a ring (a constant-Q call forks once per octave): an event is never re-recorded while the side stream may
    // still hold an unconsumed wait on its previous record -- `side_passed[i]`, recorded on the side stream right behind that wait, is synchronised
    // before slot i is used again (it has normally completed long before).  ADVICE r04: one re-recorded event let such a wait slip on ROCm 7.0.
    static constexpr int kForkRing = 16;
    hipEvent_t fork_event[kForkRing] = {}, side_passed[kForkRing] = {};
    bool fork_used[kForkRing] = {};
    int fork_next = 0;
    // join: the same treatment in the other direction -- back-to-back transforms no longer synchronise with the host between calls, so call
    // k + 1's join could re-record a single join event while the main stream's wait on call k's record is still queued.  A ring of join events;
    // `main_passed[i]`, recorded on the main stream right behind its wait, is synchronised before slot i is recorded again.
    static constexpr int kJoinRing = 8;
    hipEvent_t join_event[kJoinRing] = {}, main_passed[kJoinRing] = {};
    bool join_used[kJoinRing] = {};
    int join_next = 0;
    bool on_side = false, side_used = false;
    struct ResampleFft* rs_fft = nullptr;  // whole-signal transforms of lra_resample_fft_exec, created on first use
    int opt_pipe_chunk_mb = 128;      // bytes (in + out) one pipeline stage moves
    int opt_pipe_threads = 8;         // host threads per staging copy
};

namespace lra {

struct Scratch {
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return LRA_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        LRA_HIP(hipMalloc(&p, need));
        bytes = need;
        return LRA_OK;
    }
    ~Scratch() {
        if (p) (void)hipFree(p);
    }
};

inline int upload(void** dptr, const void* host, size_t bytes) {
    *dptr = nullptr;
    LRA_HIP(hipMalloc(dptr, bytes ? bytes : 16));
    if (bytes) LRA_HIP(hipMemcpy(*dptr, host, bytes, hipMemcpyHostToDevice));
    return LRA_OK;
}

// Every entry point runs with the context's device current and puts the caller's device back on exit: a torch
// process that calls in with cuda:0 current and a tensor on cuda:1 (or a NumPy call that defaults to LOCAL_RANK's
// device) must not find its own current device changed behind its back.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) {
            err = hipSetDevice(device);
            switched = err == hipSuccess;
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define LRA_BIND(ctxptr)                                                                                       \
    if (!(ctxptr)) return lra::fail(LRA_EINVAL, "null context");                                                    \
    lra::DeviceGuard device_guard__((ctxptr)->device);                                                              \
    if (device_guard__.err != hipSuccess) return lra::fail(LRA_EHIP, std::string("selecting the context's device: ") + hipGetErrorString(device_guard__.err))

inline size_t real_bytes(int dtype) { return dtype == LRA_F64 ? 8 : 4; }

// The double (or float) twiddle tables W_M^t, W_N^k of a mixed-radix transform length (lra_mixed.h), created on first use and kept in ctx->cqt_tw.
int ctx_twiddles(lra_ctx* ctx, int n_fft, int dtype, const void** tw_m, const void** tw_n);

// Copies the `bytes` of a small status block at `dev` (work areas start with one) to `host` and waits for the context's stream.
int read_status(lra_ctx* ctx, const void* dev, void* host, size_t bytes);

}  // namespace lra
