// lra_api.hip -- gfx950 library behind include/librosa_amd.h.
//
// Two execution paths per transform:
//   * power-of-two n_fft: the fused LDS-FFT kernels of lra_kernels.h (hand-written Stockham FFT,
//     window/pad fused into the gather, |X|^p and the banded mel reduce fused into the epilogue,
//     overlap-add with an LDS carry for the inverse);
//   * any other n_fft (the reference's tests use 501, 755, 1023, 1025, 2049): a framing kernel +
//     rocFFT batched R2C/C2R + small elementwise kernels.
// No CPU fallback exists: without a device every entry point that touches data fails.
//
// Not in this file: the entry points of the feature families that have a translation unit of their own (tempogram, beat, peaks, chroma, pitch,
// viterbi, dtw, rqa, knn, yin, pyin) are defined beside their kernels in lra_<feature>_inst.hip; lra_internal.h holds what those units share
// with this one (the context, the error macros, device binding).  The fused power-of-two kernels are declared here and compiled in lra_inst.hip.
// Comments of the form [sel:name] / [geo:name] are anchors that tests/geometry_cases.py cites in place of line numbers.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/librosa_amd.h"
#define LRA_FUSED_EXTERN  // the fused kernels are instantiated in lra_inst.hip (parallel build), see lra_fused.h
#include "lra_fused.h"
#include "lra_mel.h"
#include "lra_post.h"
#include "lra_pcen.h"
#include "lra_onset.h"
#include "lra_cqt.h"
#include "lra_hpss.h"
#include "lra_probe.h"
#include "lra_rng.h"
#include "lra_mixed_launch.h"
#include "lra_internal.h"

using namespace lra;

// ------------------------------------------------------------------------------------------------
// error plumbing (the macros: lra_internal.h)
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;  // the one error slot: every unit's failures arrive here through lra::fail

int lra::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// ------------------------------------------------------------------------------------------------
// objects (lra_ctx: lra_internal.h)
// ------------------------------------------------------------------------------------------------
// Two-slot staging between pageable host buffers and the device for the host-buffer entry points: pinned buffers the DMA
// engines read / write at link rate, device buffers that persist across calls (a streaming caller -- stft(center=False,
// out=D) per block -- allocates nothing after its first block), one stream per direction next to the compute stream.
struct HostPipe {
    size_t in_cap = 0, out_cap = 0;  // bytes per slot
    void* pin_in[2] = {nullptr, nullptr};
    void* pin_out[2] = {nullptr, nullptr};
    void* dev_in[2] = {nullptr, nullptr};
    void* dev_out[2] = {nullptr, nullptr};
    void* dev_aux = nullptr;  // small per-call table (the inverse transform's window sum-square)
    size_t aux_cap = 0;
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_comp[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
    void release_buffers(bool in, bool out) {
        for (int i = 0; i < 2; ++i) {
            if (in) {
                if (pin_in[i]) (void)hipHostFree(pin_in[i]);
                if (dev_in[i]) (void)hipFree(dev_in[i]);
                pin_in[i] = dev_in[i] = nullptr;
            }
            if (out) {
                if (pin_out[i]) (void)hipHostFree(pin_out[i]);
                if (dev_out[i]) (void)hipFree(dev_out[i]);
                pin_out[i] = dev_out[i] = nullptr;
            }
        }
        if (in) in_cap = 0;
        if (out) out_cap = 0;
    }
    ~HostPipe() {
        release_buffers(true, true);
        if (dev_aux) (void)hipFree(dev_aux);
        for (int i = 0; i < 2; ++i) {
            if (ev_in[i]) (void)hipEventDestroy(ev_in[i]);
            if (ev_comp[i]) (void)hipEventDestroy(ev_comp[i]);
            if (ev_out[i]) (void)hipEventDestroy(ev_out[i]);
        }
        if (s_in) (void)hipStreamDestroy(s_in);
        if (s_out) (void)hipStreamDestroy(s_out);
    }
};

struct lra_event {
    lra_ctx* ctx;
    hipEvent_t ev;
};

namespace {

// rocFFT plans of the general (non-power-of-two) path.  A batched plan is specific to its transform count, which is
// clips x frames of the call; so that variable-length inputs neither create a plan per call nor grow device memory
// without bound, a call runs as full chunks of kFftChunk transforms (one canonical plan) plus one remainder, and the
// cache keeps at most kMaxFftPlans plans (least recently used evicted and destroyed).
constexpr long long kFftChunk = 65536;  // (8192 made a 256-clip call 129 rocfft_execute launches: launch-bound)
constexpr size_t kMaxFftPlans = 8;
struct FftPlanCache {
    std::vector<std::pair<long long, rocfft_plan>> plans;  // most recently used last; key = number of transforms
    rocfft_execution_info info = nullptr;
    void* work = nullptr;
    size_t work_bytes = 0;
    // The frame / spectrum scratch and the work buffer belong to the plan, not to a stream: a call on another stream
    // first waits for the previous user's last kernel (event recorded at the end of every general-path call).
    hipEvent_t last_use = nullptr;
    hipStream_t last_stream = nullptr;
    ~FftPlanCache() {
        for (auto& kv : plans) rocfft_plan_destroy(kv.second);
        if (info) rocfft_execution_info_destroy(info);
        if (work) (void)hipFree(work);
        if (last_use) (void)hipEventDestroy(last_use);
    }
};

std::once_flag g_rocfft_once;
void rocfft_setup_once() {
    std::call_once(g_rocfft_once, [] { rocfft_setup(); });
}

}  // namespace

struct lra_stft_plan {
    lra_ctx* ctx = nullptr;
    int n_fft = 0, hop = 0, center = 0, pad_mode = 0, dtype = 0;
    bool pow2 = false;
    int logm = 0;
    void* d_win = nullptr;
    void* d_win_full = nullptr;  // powers of two in lra_mixed_sizes.h's forward list: the window itself (d_win holds 0.5 x window there), for the flat-index mel kernel
    void* d_tw[kNumVariants] = {};
    int tuned_variant[4] = {-1, -1, -1, -1};  // per epilogue mode (autotune), -1 = not measured yet  // pass-twiddle tables; their layout depends on the kernel configuration
    void* d_twr = nullptr;
    FftPlanCache fft;
    Scratch frames, spec;
    // mixed-radix fused path (lra_mixed.h): W_M^t (M entries) and W_N^k (M + 1 entries); null when n_fft is not in its size list
    void* d_mtw = nullptr;
    void* d_mtwn = nullptr;
};

struct lra_mel_plan {
    lra_ctx* ctx = nullptr;
    int n_mels = 0, n_bins = 0, dtype = 0;
    int* d_c0 = nullptr;
    int* d_len = nullptr;
    int* d_off = nullptr;
    void* d_val = nullptr;
    int nnz = 0;  // weights in d_val
    // two-slope form (lra_mel.h); two_slope == false -> only the generic banded path is available
    bool two_slope = false;
    void* d_wAB = nullptr;
    // piece tables for runs of 8 / 16 bins per thread (index 0 / 1); n_pieces == 0 -> not available
    // run-ordered form (OUT_MELR; 16 points per thread: TF = M/16 threads per frame, runs of 8 bins)
    void* d_melr_w = nullptr;
    void* d_melr_keep = nullptr;
    int* d_melr_addr = nullptr;
    int melr_zero = 0, melr_mid = 0, melr_pmax = 0;
    bool melr_ok = false;
    bool melr_many = false;  // the layout-0 tables were built for the many-bands kernel shape (lra_dispatch.h, MelManyCfgOf: eight bands, one hoisted piece per list)
    // the same for the second-generation kernel (lra_mel.h layout 1: both runs ascending, extra bin M)
    void* d_melr2_w = nullptr;
    void* d_melr2_keep = nullptr;
    int* d_melr2_addr = nullptr;
    int melr2_zero = 0, melr2_mid = 0, melr2_pmax = 0;
    bool melr2_ok = false;
    int* d_run[2] = {nullptr, nullptr};
    int* d_segd[2] = {nullptr, nullptr};
    int nyq[2] = {0, 0};
    int n_pieces[2] = {0, 0};
};

struct lra_istft_plan {
    lra_ctx* ctx = nullptr;
    int n_fft = 0, hop = 0, center = 0, dtype = 0;
    bool pow2 = false;
    int logm = 0;
    void* d_win_scaled = nullptr;  // window / n_fft
    void* d_tw[kNumVariants] = {};
    int tuned_variant[4] = {-1, -1, -1, -1};  // per epilogue mode (autotune), -1 = not measured yet
    void* d_twr = nullptr;
    FftPlanCache fft;
    Scratch spec, frames;
    Scratch norm;  // lra_istft_exec: 1 / wss of the call's envelope (the kernels multiply; see istft_run)
    void* d_mtw = nullptr;   // mixed-radix inverse (lra_mixed.h): W_M^t, W_N^k; null when n_fft is not in its size list
    void* d_mtwn = nullptr;
};

namespace {

// resident workgroups per CU of a kernel at a given dynamic LDS size (cached; 0 = unknown)
static int resident_workgroups(const void* kern, int block, int lds) {
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, int> cache;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_pair(kern, lds);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int per_cu = 0;
    if (lds > 65536) (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, block, lds) != hipSuccess) per_cu = 0;
    (void)hipGetLastError();
    cache[key] = per_cu;
    return per_cu;
}

template <class T> struct StftLaunch {
    StftArgs<T> a;
    int mode = 0;
    long long batch = 0;
    int iters_opt = 0;  // 0 = auto
    int mel_tile_opt = 0;
    int n_cu = 256;
    void* out = nullptr;
    int lds_pad = 0;
    bool xcd_remap = true;
    bool use_v2 = true;
    bool use_direct = true;
    bool mel_v2 = false;  // OUT_MELR: the plan's layout-1 tables are bound, run the second-generation kernel
    bool mel_pc = false;  // fused mel: the producer / consumer kernel where it applies (lra_kernels_pc.h)
    bool mel_runs = true;
    const lra_mel_plan* mel = nullptr;
    hipStream_t stream = nullptr;
    hipError_t err = hipSuccess;

    // The instance of a kernel family for the call's power mode; `inst(pm)` names the instance of compile-time power mode decltype(pm)::value.  The complex
    // epilogue raises nothing to a power and exists as POW_TWO only, so nothing else is named for it (a named instance has to be in lra_fused.h's lists).
    using Kern = void (*)(StftArgs<T>, const T*, void*);
    template <int MODE, class F> Kern pick_power(F inst) const {
        if constexpr (MODE != OUT_COMPLEX) {
            if (a.power_mode == POW_ONE) return inst(std::integral_constant<int, POW_ONE>{});
            if (a.power_mode == POW_GENERAL) return inst(std::integral_constant<int, POW_GENERAL>{});
        }
        return inst(std::integral_constant<int, POW_TWO>{});
    }
    template <class Cfg, int MODE, int RA> Kern ring_kernel() const {
        return pick_power<MODE>([](auto pm) -> Kern { return stft_kernel<Cfg, MODE, decltype(pm)::value, RA>; });
    }
    template <class Cfg, int HD, int MODE> Kern v2_kernel() const {
        return pick_power<MODE>([](auto pm) -> Kern { return stft2_kernel<Cfg, HD, MODE, decltype(pm)::value>; });
    }

    template <class Cfg, int MODE> void launch(int shared_bytes) {
        static_assert(Cfg::P <= 4, "at most four Stockham passes are wired up");
        const int lds_probe_v1 = Cfg::FPB * stft_slot_bytes<Cfg>(MODE, a.n_mels, mel_tile_opt > 0 ? mel_tile_opt : 4) + shared_bytes + lds_pad;
        Kern kern = nullptr;
        bool direct = false;
        if constexpr (Cfg::PLAN == 0) {  // (the radix 16-16-4 configuration has second-generation instances only)
        kern = ring_kernel<Cfg, MODE, 0>();  // [sel:ring]
        if constexpr (sizeof(T) == 4) {  // row-aligned hops (n_fft/4, n_fft/8, ...): the fast ring addressing, f32 only  // [sel:ringrows-f32]
            if (ring_rows_aligned<Cfg>(a.hop)) kern = ring_kernel<Cfg, MODE, 1>();  // [sel:ringrows]
        }
        // hop >= n_fft (frames do not overlap): direct framing, no ring (complex / power epilogues)
        if constexpr (MODE == OUT_COMPLEX || MODE == OUT_POWER) {
            if (a.hop >= Cfg::N && use_direct) {  // [sel:direct]
                direct = true;
                kern = ring_kernel<Cfg, MODE, 2>();
            }
        }
        // n_fft >= 8192 (f32) with hop = n_fft / {2, 4, 8, 16}: the sample ring lives in registers (RA = 2 + log2 HD)
        if constexpr ((MODE == OUT_COMPLEX || MODE == OUT_POWER) && sizeof(T) == 4 && (Cfg::LOGM >= 12 || Cfg::LOGM == 7 || Cfg::LOGM == 8)) {
            const int hd = use_direct ? regring_hd<Cfg>(a.hop) : 0;  // [sel:regring]
            if (hd) direct = true;
            if (hd == 2) kern = ring_kernel<Cfg, MODE, 3>();
            else if (hd == 4) kern = ring_kernel<Cfg, MODE, 4>();
            else if (hd == 8) kern = ring_kernel<Cfg, MODE, 5>();
            else if (hd == 16) kern = ring_kernel<Cfg, MODE, 6>();
        }
        }
        // Second-generation kernel (lra_kernels2.h) where it applies: complex / power epilogues, 16 points per thread with
        // a two-butterfly last pass (n_fft 1024 / 2048 / 4096 / 16384), hop = n_fft / {1, 2, 4, 8}.
        bool v2 = false;
        if constexpr (v23_cfg_ok<Cfg>() && (MODE == OUT_COMPLEX || MODE == OUT_POWER || MODE == OUT_MELR)) {
            const int hd = (use_v2 && (MODE != OUT_MELR || mel_v2)) ? v2_hop_divisor<Cfg>(a.hop) : 0;
            if (hd) {  // [sel:v2]
                v2 = true;
                kern = hd == 1 ? v2_kernel<Cfg, 1, MODE>() : hd == 2 ? v2_kernel<Cfg, 2, MODE>() : hd == 4 ? v2_kernel<Cfg, 4, MODE>() : v2_kernel<Cfg, 8, MODE>();
            }
        }
        if (!kern) { err = hipErrorInvalidValue; return; }
        const int lds_probe = v2 ? Cfg::FPB * stft2_slot_bytes<Cfg>() + shared_bytes + lds_pad : direct ? Cfg::FPB * Cfg::FRAME_BYTES + lds_pad : lds_probe_v1;
        // Frames per slot (`iters`).  A slot pays n_fft - hop extra sample loads for its first frame, so long
        // runs are cheap in HBM traffic; but the launch should also end evenly: the grid is sized to a whole
        // number of "waves" of workgroups (CUs x resident workgroups per CU), because a last partial wave
        // leaves most of the chip idle for one workgroup's duration (~15 % of a 0.85 ms launch at 32 frames
        // per slot on the 256 x 30 s batch).  Among 24..176 frames per slot, take the best fill, then the
        // longest run.
        int iters = iters_opt;
        if (iters <= 0) {
            const int per_cu = lds_probe <= 160 * 1024 ? resident_workgroups(reinterpret_cast<const void*>(kern), Cfg::NT, lds_probe) : 0;
            const long long conc = (long long)n_cu * (per_cu > 0 ? per_cu : 1);
            const int fpb = Cfg::FPB;
            int best_iters = 0;
            double best_fill = -1.0;
            for (int cand = 176; cand >= 24; --cand) {
                const int wgpc = (a.n_frames + fpb * cand - 1) / (fpb * cand);
                const int it = (a.n_frames + fpb * wgpc - 1) / (fpb * wgpc);  // equal shares
                const double rounds = (double)(batch * wgpc) / (double)conc;
                // a single round that occupies at least 60 % of the slots has no tail to speak of, and long runs beat full
                // residency there (measured on the 256 x 30 s batch: 162 frames per slot 0.657 ms, 108 0.674, 324 0.674)
                // (that kernel is bound by its store stream; the others -- small frames sharing a wave, frames spread over
                // several waves -- are bound by latency and want every resident slot taken: n_fft = 512, hop = 512 ran 5 of 8
                // resident workgroups per CU under this rule)
                const double fill = (v2 && Cfg::TF == 64 && rounds <= 1.0 && rounds >= 0.6) ? 1.0 : rounds / std::ceil(rounds);
                if (fill > best_fill + 0.02) { best_fill = fill; best_iters = it; }
            }
            iters = best_iters;
            // small jobs: keep at least ~2 workgroups per CU even if that means short runs
            while (iters > 4 && batch * ((a.n_frames + fpb * iters - 1) / (fpb * iters)) < 2LL * n_cu) iters /= 2;
        }
        if (iters < 1) iters = 1;
        // several slots per wave (n_fft < 2048) with the row-aligned ring: keep the slots in step (frames per slot a
        // multiple of n_fft / hop = 4) so that the ring rotation is one scalar per wave
        a.rot_uniform = 0;
        if (Cfg::FPB > 1 && Cfg::TF < 64 && ring_rows_aligned<Cfg>(a.hop)) {  // [geo:rot-uniform]
            if (iters_opt <= 0 && iters >= 4) iters = (iters + 3) / 4 * 4;
            a.rot_uniform = iters % 4 == 0;
        }
        a.mel_tile = mel_tile_opt > 0 ? mel_tile_opt : 4;
        if (a.mel_tile > iters) a.mel_tile = iters;  // [geo:mel-tile]
        a.frames_per_wg = Cfg::FPB * iters;  // [geo:strips]
        a.wg_per_clip = (a.n_frames + a.frames_per_wg - 1) / a.frames_per_wg;
        a.slot_bytes = v2 ? stft2_slot_bytes<Cfg>() : direct ? Cfg::FRAME_BYTES : stft_slot_bytes<Cfg>(MODE, a.n_mels, a.mel_tile);
        a.shared_off = Cfg::FPB * a.slot_bytes;
        const long long grid = batch * a.wg_per_clip;
        if (grid > 0x7ffffff0LL) { err = hipErrorInvalidConfiguration; return; }
        const int lds = Cfg::FPB * a.slot_bytes + shared_bytes + lds_pad;  // lds_pad: occupancy experiments only
        if (lds > 160 * 1024) { err = hipErrorInvalidValue; return; }
        if (lds > 65536) {
            err = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
            if (err != hipSuccess) return;
        }
        a.n_blocks = (int)grid;
        a.xcd_chunk = (xcd_remap && grid >= 64) ? (int)((grid + 7) / 8) : 0;  // [geo:xcd-pad]
        const long long launch_grid = a.xcd_chunk ? 8LL * a.xcd_chunk : grid;
        hipLaunchKernelGGL(kern, dim3((unsigned)launch_grid), dim3(Cfg::NT), lds, stream, a, a.y, out);
        err = hipGetLastError();
    }

    // Producer / consumer fused mel kernel (lra_kernels_pc.h): 192-thread workgroups [P, P, C], NP = 2 frame slots each.  Geometry as above:
    // strips of 24..176 frames per slot, the grid a whole number of rounds of resident workgroups (four per CU).
    template <class Cfg> void launch_pc(int hd) {  // [sel:launch-pc]
        using PL = PcLayout<Cfg>;
        const Kern kern = hd == 4 ? pick_power<OUT_MEL2>([](auto pm) -> Kern { return stft_pc_kernel<Cfg, 4, decltype(pm)::value>; })
                                  : pick_power<OUT_MEL2>([](auto pm) -> Kern { return stft_pc_kernel<Cfg, 8, decltype(pm)::value>; });
        const int lds = PL::BYTES + lds_pad;
        constexpr int fpb = PL::NP;  // [geo:pc-np]
        int iters = iters_opt;
        if (iters <= 0) {
            const int per_cu = resident_workgroups(reinterpret_cast<const void*>(kern), PL::NT, lds);
            const long long conc = (long long)n_cu * (per_cu > 0 ? per_cu : 1);
            int best_iters = 0;
            double best_fill = -1.0;
            for (int cand = 176; cand >= 24; --cand) {
                const int wgpc = (a.n_frames + fpb * cand - 1) / (fpb * cand);
                const int it = (a.n_frames + fpb * wgpc - 1) / (fpb * wgpc);
                const double rounds = (double)(batch * wgpc) / (double)conc;
                const double fill = (rounds <= 1.0 && rounds >= 0.6) ? 1.0 : rounds / std::ceil(rounds);
                if (fill > best_fill + 0.02) { best_fill = fill; best_iters = it; }
            }
            iters = best_iters;
            while (iters > 4 && batch * ((a.n_frames + fpb * iters - 1) / (fpb * iters)) < 2LL * n_cu) iters /= 2;
        }
        if (iters < 1) iters = 1;
        a.rot_uniform = 0;
        a.mel_tile = 1;
        a.frames_per_wg = fpb * iters;  // [geo:pc-strips]
        a.wg_per_clip = (a.n_frames + a.frames_per_wg - 1) / a.frames_per_wg;
        a.slot_bytes = PL::FRAME;
        a.shared_off = 0;
        const long long grid = batch * a.wg_per_clip;
        if (grid > 0x7ffffff0LL) { err = hipErrorInvalidConfiguration; return; }
        a.n_blocks = (int)grid;
        a.xcd_chunk = (xcd_remap && grid >= 64) ? (int)((grid + 7) / 8) : 0;  // [geo:pc-xcd-pad]
        const long long launch_grid = a.xcd_chunk ? 8LL * a.xcd_chunk : grid;
        hipLaunchKernelGGL(kern, dim3((unsigned)launch_grid), dim3(PL::NT), lds, stream, a, a.y, out);
        err = hipGetLastError();
    }

    template <class Cfg> void operator()() {
        if constexpr (Cfg::REV) {  // the ascending-radix configurations exist for the inverse kernel only
            err = hipErrorInvalidValue;
            return;
        } else if constexpr (Cfg::PLAN == 1) {  // radices 16, 16, 4: second-generation kernels only (stft_run selects the variant where they apply)  // [sel:plan1]
            if (!use_v2 || v2_hop_divisor<Cfg>(a.hop) == 0) { err = hipErrorInvalidValue; return; }
            if (mode == OUT_COMPLEX) launch<Cfg, OUT_COMPLEX>(0);
            else if (mode == OUT_POWER) launch<Cfg, OUT_POWER>(0);
            else if (mode == OUT_MEL2 && mel_pc && mel && mel->melr2_ok && mel_runs) {  // the producer / consumer mel kernel on this core (ctx option mel_pc = 2)
                if constexpr (pc_cfg_ok<Cfg>()) {
                    const int hd_pc = v2_hop_divisor<Cfg>(a.hop);
                    if (!pc_bank_ok<Cfg>(a.n_mels, mel->melr2_pmax) || !pc_fits_budget<Cfg>(hd_pc, a.power_mode)) { err = hipErrorInvalidValue; return; }
                    a.melr_w = (const T*)mel->d_melr2_w;
                    a.melr_keep = (const T*)mel->d_melr2_keep;
                    a.melr_addr = mel->d_melr2_addr;
                    a.melr_zero = mel->melr2_zero;
                    a.melr_mid = mel->melr2_mid;
                    a.melr_pmax = mel->melr2_pmax;
                    launch_pc<Cfg>(hd_pc);
                } else err = hipErrorInvalidValue;
            } else err = hipErrorInvalidValue;
        } else {
            run<Cfg>();
        }
    }
    template <class Cfg> void run() {
        if (mode == OUT_MEL2) {
            // the two-slope mel kernel shares its filter tables across the slots of a larger workgroup
            using MC = typename MelCfgOf<Cfg>::type;
            // n_fft = 2048, float32, banks of up to 128 bands with pair segments of at most four pieces: producer and consumer waves (lra_kernels_pc.h)
            if constexpr (pc_cfg_ok<Cfg>()) {
                const int hd_pc = v2_hop_divisor<Cfg>(a.hop);
                if (mel_pc && mel && mel->melr2_ok && mel_runs && use_v2 && pc_bank_ok<Cfg>(a.n_mels, mel->melr2_pmax) && pc_fits_budget<Cfg>(hd_pc, a.power_mode)) {  // [sel:mel-pc]
                    a.melr_w = (const T*)mel->d_melr2_w;
                    a.melr_keep = (const T*)mel->d_melr2_keep;
                    a.melr_addr = mel->d_melr2_addr;
                    a.melr_zero = mel->melr2_zero;
                    a.melr_mid = mel->melr2_mid;
                    a.melr_pmax = mel->melr2_pmax;
                    launch_pc<Cfg>(hd_pc);
                    return;
                }
            }
            // first choice: the run-ordered form (no per-lane control flow, no (wA P, wB P) round trip through LDS)
            if constexpr (v2_cfg_ok<MC>()) {
                if (mel && mel->melr2_ok && mel_runs && use_v2 && melr_fits<MC>() && v2_hop_divisor<MC>(a.hop) > 0) {  // [sel:mel-onewave]
                    const int shared_r = melr_shared_bytes<MC>(a.n_mels, mel->melr2_pmax);
                    if (MC::FPB * stft2_slot_bytes<MC>() + shared_r <= 160 * 1024) {
                        a.melr_w = (const T*)mel->d_melr2_w;
                        a.melr_keep = (const T*)mel->d_melr2_keep;
                        a.melr_addr = mel->d_melr2_addr;
                        a.melr_zero = mel->melr2_zero;
                        a.melr_mid = mel->melr2_mid;
                        a.melr_pmax = mel->melr2_pmax;
                        mel_v2 = true;
                        mel_tile_opt = 1;
                        launch<MC, OUT_MELR>(shared_r);
                        return;
                    }
                }
            }
            if constexpr (mel_many_applies<Cfg>()) {
                using MM = typename MelManyCfgOf<Cfg>::type;
                if (mel && mel->melr_ok && mel->melr_many && mel_runs && melr_fits<MM>()) {  // [sel:mel-many]
                    const int shared_m = melr_shared_bytes<MM>(a.n_mels, mel->melr_pmax);
                    if (MM::FPB * stft_slot_bytes<MM>(OUT_MELR, a.n_mels, 1) + shared_m <= 160 * 1024) {
                        a.melr_w = (const T*)mel->d_melr_w;
                        a.melr_keep = (const T*)mel->d_melr_keep;
                        a.melr_addr = mel->d_melr_addr;
                        a.melr_zero = mel->melr_zero;
                        a.melr_mid = mel->melr_mid;
                        a.melr_pmax = mel->melr_pmax;
                        mel_tile_opt = 1;
                        launch<MM, OUT_MELR>(shared_m);
                        return;
                    }
                }
            }
            if (mel && mel->melr_ok && !mel->melr_many && mel_runs && melr_fits<MC>() && MC::R == 16) {  // [sel:mel-runs]
                const int shared_r = melr_shared_bytes<MC>(a.n_mels, mel->melr_pmax);
                // no LDS staging tile by default: the kernel keeps the last 8 frames of each band in registers and stores them as one burst
                int tile_r = mel_tile_opt > 0 ? mel_tile_opt : 1;
                while (tile_r > 1 && MC::FPB * stft_slot_bytes<MC>(OUT_MELR, a.n_mels, tile_r) + shared_r > 160 * 1024) tile_r /= 2;
                if (MC::FPB * stft_slot_bytes<MC>(OUT_MELR, a.n_mels, tile_r) + shared_r <= 160 * 1024) {
                    a.melr_w = (const T*)mel->d_melr_w;
                    a.melr_keep = (const T*)mel->d_melr_keep;
                    a.melr_addr = mel->d_melr_addr;
                    a.melr_zero = mel->melr_zero;
                    a.melr_mid = mel->melr_mid;
                    a.melr_pmax = mel->melr_pmax;
                    mel_tile_opt = tile_r;
                    launch<MC, OUT_MELR>(shared_r);
                    return;
                }
            }
            const int shared = mel2_shared_bytes<MC>(a.n_mels);
            // largest staging tile (frames per flushed mel row) that still fits the 160 KiB of LDS
            int tile = mel_tile_opt > 0 ? mel_tile_opt : 4;  // [geo:staging-tile]
            while (tile > 1 && MC::FPB * stft_slot_bytes<MC>(OUT_MEL2, a.n_mels, tile) + shared > 160 * 1024) tile /= 2;
            const int pi = MC::R == 16 ? 1 : 0;
            if (mel && mel2_fits<MC>(a.n_mels) && mel->n_pieces[pi] > 0 && mel->n_pieces[pi] <= MC::TF + a.n_mels + 2 &&  // [sel:mel-masked]
                MC::FPB * stft_slot_bytes<MC>(OUT_MEL2, a.n_mels, tile) + shared <= 160 * 1024) {
                a.mel_run = mel->d_run[pi];
                a.mel_segd = mel->d_segd[pi];
                a.mel_nyq = mel->nyq[pi];
                mel_tile_opt = tile;
                launch<MC, OUT_MEL2>(shared);
                return;
            }
            launch<Cfg, OUT_MEL>(0);  // generic banded path  // [sel:mel-generic]
            return;
        }
        if (mode == OUT_COMPLEX) launch<Cfg, OUT_COMPLEX>(0);
        else if (mode == OUT_POWER) launch<Cfg, OUT_POWER>(0);
        else launch<Cfg, OUT_MEL>(0);
    }
};

template <class T> struct IstftLaunch {
    IstftArgs<T> a;
    long long batch = 0;
    int strip_frames = 0;  // 0 = auto
    int n_cu = 256;
    bool xcd_remap = true;
    bool too_big = false;  // the slot does not fit the 160 KiB of LDS (n_fft = 16384 with a hop outside n_fft/2, /4, /8): caller takes the rocFFT path
    hipStream_t stream = nullptr;
    hipError_t err = hipSuccess;
    template <class Cfg> void operator()() {
        if constexpr (Cfg::PLAN == 1 && !Cfg::REV) {  // forward-only configuration (radices 16, 16, 4)
            err = hipErrorInvalidValue;
            return;
        } else if constexpr (Cfg::PLAN == 1) {  // radices 4, 16, 16: the row-aligned overlap-add forms only (instances: HC = 8, 4, 2, 1)  // [sel:istft-plan1]
            if (istft_rows_hc<Cfg>(a.hop) == 0) { err = hipErrorInvalidValue; return; }
            run<Cfg>();
        } else {
            run<Cfg>();
        }
    }
    template <class Cfg> void run() {
        static_assert(Cfg::P <= 4, "at most four Stockham passes are wired up");
        constexpr int FPB = Cfg::FPB, N = Cfg::N;
        const int H = a.hop;
        a.warm_frames = (N + H - 1) / H - 1;
        a.drain_steps = N > H ? (N - H + H - 1) / H : 0;
        a.batch = batch;
        int lds = istft_lds_bytes<Cfg, 0>();
        void (*kern)(IstftArgs<T>, const cx<T>*, const T*, T*) = istft_kernel<Cfg, 0>;  // [sel:istft-general]
        if constexpr (sizeof(T) == 4) {  // row-aligned overlap-add for hop = n_fft/2, n_fft/4 and n_fft/8 (f32)  // [sel:istft-rows]
            const int hc = istft_rows_hc<Cfg>(a.hop);
            if constexpr (Cfg::R >= 4) {
                if (hc == Cfg::R / 2) { kern = istft_kernel<Cfg, Cfg::R / 2>; lds = istft_lds_bytes<Cfg, Cfg::R / 2>(); }
                if (hc == Cfg::R / 4) { kern = istft_kernel<Cfg, Cfg::R / 4>; lds = istft_lds_bytes<Cfg, Cfg::R / 4>(); }
            }
            if constexpr (Cfg::R >= 8) {
                if (hc == Cfg::R / 8) { kern = istft_kernel<Cfg, Cfg::R / 8>; lds = istft_lds_bytes<Cfg, Cfg::R / 8>(); }
            }
            if constexpr (Cfg::R >= 16) {
                if (hc == Cfg::R / 16) { kern = istft_kernel<Cfg, Cfg::R / 16>; lds = istft_lds_bytes<Cfg, Cfg::R / 16>(); }
            }
        }
        if (lds > 160 * 1024) { too_big = true; return; }
        // Frames per strip.  Each strip replays warm_frames frames before its own, so long strips are cheap;
        // like the forward kernel, the grid should be a whole number of resident waves of workgroups.
        int sf = strip_frames;
        if (sf <= 0) {
            const int per_cu = resident_workgroups(reinterpret_cast<const void*>(kern), Cfg::NT, lds);
            const long long conc = (long long)n_cu * (per_cu > 0 ? per_cu : 1);
            double best_fill = -1.0;
            sf = 64;
            for (int cand = 176; cand >= 32; --cand) {  // (up to 1292 / 8 = 162 frames for the 30 s clips of BASELINE: one round of strips, 1.9 % of warm-up reads)
                const int spc = (a.n_used + cand - 1) / cand;
                const int fr = (a.n_used + spc - 1) / spc;  // equal shares
                const double rounds = (double)((batch * spc + FPB - 1) / FPB) / (double)conc;
                const double fill = rounds / std::ceil(rounds);
                if (fill > best_fill + 0.02) { best_fill = fill; sf = fr; }
            }
            while (sf > 8 && (batch * ((a.n_used + sf - 1) / sf) + FPB - 1) / FPB < 2LL * n_cu) sf /= 2;  // small jobs: fill the chip first
        }
        a.strip_frames = sf < 1 ? 1 : sf;  // [geo:istft-strips]
        a.strips_per_clip = (a.n_used + a.strip_frames - 1) / a.strip_frames;
        const long long grid = (batch * a.strips_per_clip + FPB - 1) / FPB;
        if (grid > 0x7ffffff0LL) { err = hipErrorInvalidConfiguration; return; }
        if (lds > 65536) {
            err = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
            if (err != hipSuccess) return;
        }
        a.n_blocks = (int)grid;
        a.xcd_chunk = (xcd_remap && grid >= 64) ? (int)((grid + 7) / 8) : 0;  // [geo:istft-xcd-pad]
        const long long launch_grid = a.xcd_chunk ? 8LL * a.xcd_chunk : grid;
        hipLaunchKernelGGL(kern, dim3((unsigned)launch_grid), dim3(Cfg::NT), lds, stream, a, a.D, a.wss, a.y);
        err = hipGetLastError();
    }
};

template <class T> struct TableBuild {
    std::vector<cx<T>> tw, twr;
    template <class Cfg> void operator()() {
        tw.assign(Cfg::TW_TOTAL, mk<T>((T)1, (T)0));
        twr.assign(split_tw_count<Cfg>(), mk<T>((T)1, (T)0));
        build_pass_twiddles<Cfg>(tw.data());
        build_split_twiddles<Cfg>(twr.data());
    }
};

template <class T> int build_tables(int logm, void** d_tw /* [kNumVariants] */, void** d_twr) {
    for (int v = 0; v < kNumVariants; ++v) {
        TableBuild<T> tb;
        if (!dispatch_logm<T>(logm, v, tb)) return fail(LRA_EINVAL, "unsupported power-of-two size");
        LRA_TRY(upload(&d_tw[v], tb.tw.data(), tb.tw.size() * sizeof(cx<T>)));
        if (v == 0) LRA_TRY(upload(d_twr, tb.twr.data(), tb.twr.size() * sizeof(cx<T>)));
    }
    return LRA_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// kernels: general (rocFFT) path and helpers
// ------------------------------------------------------------------------------------------------
// frames[f][i] = win[i] * ypad[clip][t*hop - pad + i], f = (clip - clip0)*n_frames + t
template <class T>
__global__ void frame_window_kernel(const T* __restrict__ y, long long y_stride, long long n, int n_frames, int hop, int pad, int pad_mode,
                                    const T* __restrict__ win, int N, long long clip0, long long total_frames, T* __restrict__ out) {
    const int chunks = (N + 255) / 256;
    const long long f = blockIdx.x / chunks;
    const int i = (int)(blockIdx.x % chunks) * 256 + threadIdx.x;
    if (f >= total_frames || i >= N) return;
    const long long clip = clip0 + f / n_frames;
    const long long t = f % n_frames;
    const long long g = t * hop - pad + i;
    const long long idx = pad_index(g, n, pad_mode);
    const T v = idx >= 0 ? y[clip * y_stride + idx] : (T)0;
    out[f * N + i] = v * win[i];
}

template <class T> __global__ void power_kernel(const cx<T>* __restrict__ D, T* __restrict__ S, long long count, int power_mode, T power) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    if (power_mode == POW_TWO) S[i] = spec_power<T, POW_TWO>(D[i], power);
    else if (power_mode == POW_ONE) S[i] = spec_power<T, POW_ONE>(D[i], power);
    else S[i] = spec_power<T, POW_GENERAL>(D[i], power);
}

// General mel path: S^T[b][f][t] = |D[b][t][f]|^power through a 32 x 33 LDS tile, so that both the read of D (lanes along f)
// and mel_apply_kernel's reads of S (lanes along t) are coalesced; with S in D's [t][f] layout the band sums read one
// element per 4 (bins + 1) bytes.
template <class T> __global__ void power_transpose_kernel(const cx<T>* __restrict__ D, T* __restrict__ St, long long n_frames, long long bins, int power_mode, T power) {
    __shared__ T tile[32][33];
    const long long b = blockIdx.z;
    const long long t0 = (long long)blockIdx.y * 32, f0 = (long long)blockIdx.x * 32;
    const cx<T>* __restrict__ d = D + b * n_frames * bins;
    T* __restrict__ s = St + b * n_frames * bins;
    for (int j = threadIdx.y; j < 32; j += 8) {
        const long long t = t0 + j, f = f0 + threadIdx.x;
        if (t < n_frames && f < bins) {
            const cx<T> z = d[t * bins + f];
            tile[j][threadIdx.x] = power_mode == POW_TWO ? spec_power<T, POW_TWO>(z, power) : power_mode == POW_ONE ? spec_power<T, POW_ONE>(z, power) : spec_power<T, POW_GENERAL>(z, power);
        }
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += 8) {
        const long long f = f0 + j, t = t0 + threadIdx.x;
        if (f < bins && t < n_frames) s[f * n_frames + t] = tile[threadIdx.x][j];
    }
}

// M[b][m][t] = sum_i val[off[m]+i] * S[b*bs + (c0[m]+i)*fs_bin + t*fs_frame]
template <class T>
__global__ void mel_apply_kernel(const T* __restrict__ S, long long batch_stride, long long bin_stride, long long frame_stride, long long n_frames,
                                 int n_mels, const int* __restrict__ c0, const int* __restrict__ len, const int* __restrict__ off,
                                 const T* __restrict__ val, T* __restrict__ Mout) {
    const long long tblocks = (n_frames + 255) / 256;
    const long long bm = blockIdx.x / tblocks;
    const long long t = (blockIdx.x % tblocks) * 256 + threadIdx.x;
    if (t >= n_frames) return;
    const int m = (int)(bm % n_mels);
    const long long b = bm / n_mels;
    const T* __restrict__ src = S + b * batch_stride + (long long)c0[m] * bin_stride + t * frame_stride;
    const T* __restrict__ w = val + off[m];
    const int L = len[m];
    T acc = (T)0;
    for (int i = 0; i < L; ++i) acc += w[i] * src[(long long)i * bin_stride];
    Mout[(b * n_mels + m) * n_frames + t] = acc;
}

// copies [clip][t][k] (strided) into a packed [f][bins] buffer and clears the imaginary parts that
// a real inverse transform ignores (DC always, Nyquist for even n_fft), as pocketfft's c2r does
template <class T>
__global__ void spec_pack_kernel(const cx<T>* __restrict__ D, long long d_batch_stride, long long d_frame_stride, int n_used, int bins, int even,
                                 long long clip0, long long total_frames, cx<T>* __restrict__ out) {
    const int chunks = (bins + 255) / 256;
    const long long f = blockIdx.x / chunks;
    const int k = (int)(blockIdx.x % chunks) * 256 + threadIdx.x;
    if (f >= total_frames || k >= bins) return;
    const long long clip = clip0 + f / n_used;
    const long long t = f % n_used;
    cx<T> v = D[clip * d_batch_stride + t * d_frame_stride + k];
    if (k == 0 || (even && k == bins - 1)) v.y = (T)0;
    out[f * bins + k] = v;
}

// gather overlap-add: y[clip][s] = sum_t ws[s' - tH] * x[f(clip,t)][s' - tH] (increasing t), / wss
// window sum-square envelope -> per-sample normalisation factor: 1 / wss where wss > tiny, else 1 (core/spectrum.py:622-624 as a product)
template <class T> __global__ void wss_to_norm_kernel(const T* __restrict__ wss, T tinyv, T* __restrict__ nrm, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const T w = wss[i];
        nrm[i] = w > tinyv ? (T)1 / w : (T)1;
    }
}

template <class T>
__global__ void ola_gather_kernel(const T* __restrict__ x, int N, int hop, int n_used, int drop, const T* __restrict__ ws, const T* __restrict__ wss, int wss_is_norm,
                                  T tinyv, long long clip0, long long clips, T* __restrict__ y, long long y_stride, long long out_len) {
    const long long chunks = (out_len + 255) / 256;
    const long long c = blockIdx.x / chunks;
    const long long s = (blockIdx.x % chunks) * 256 + threadIdx.x;
    if (c >= clips || s >= out_len) return;
    const long long sp = s + drop;
    long long t_lo = sp - N + 1;
    t_lo = t_lo <= 0 ? 0 : (t_lo + hop - 1) / hop;
    long long t_hi = sp / hop;
    if (t_hi > n_used - 1) t_hi = n_used - 1;
    T acc = (T)0;
    for (long long t = t_lo; t <= t_hi; ++t) {
        const long long off = sp - t * hop;
        acc += ws[off] * x[(c * n_used + t) * N + off];
    }
    const T w = wss[s];
    y[(clip0 + c) * y_stride + s] = wss_is_norm ? acc * w : ((w > tinyv) ? acc / w : acc);
}

// The same sums, four output samples per thread (256 apart: every load instruction stays coalesced) with 32-bit position arithmetic, the frames of all four walked
// together so that up to eight loads are in flight per trip, the normalisation factors fetched up front (round 6: the one-sample form waited 0.79 of its wave cycles
// and ran at 1.5 TB/s; it stays for signals of 2^31 samples and more).
template <class T>
__global__ __launch_bounds__(256) void ola_gather4_kernel(const T* __restrict__ x, int N, int hop, int n_used, int drop, const T* __restrict__ ws, const T* __restrict__ wss, int wss_is_norm,
                                                          T tinyv, long long clip0, long long clips, T* __restrict__ y, long long y_stride, unsigned out_len, unsigned chunks) {
    const long long c = blockIdx.x / chunks;
    const unsigned s0 = (blockIdx.x % chunks) * 1024u + threadIdx.x;
    if (c >= clips) return;
    const T* __restrict__ xc = x + c * (long long)n_used * N;
    unsigned t_lo[4], cnt[4];
    T w[4], acc[4];
    unsigned most = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const unsigned s = s0 + u * 256u;
        const bool ok = s < out_len;
        const unsigned sp = (ok ? s : 0u) + (unsigned)drop;
        const unsigned lo = sp + 1u <= (unsigned)N ? 0u : (sp + 1u - (unsigned)N + (unsigned)hop - 1u) / (unsigned)hop;
        unsigned hi = sp / (unsigned)hop;
        if (hi > (unsigned)n_used - 1u) hi = (unsigned)n_used - 1u;
        t_lo[u] = lo;
        cnt[u] = ok && hi >= lo ? hi - lo + 1u : 0u;
        most = cnt[u] > most ? cnt[u] : most;
        w[u] = wss[ok ? s : 0u];
        acc[u] = (T)0;
    }
    for (unsigned j = 0; j < most; ++j) {
        T a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool on = j < cnt[u];  // (a finished or empty sum re-reads element 0 of frame 0: always there, never used)
            const unsigned t = on ? t_lo[u] + j : 0u;
            const unsigned off = on ? s0 + u * 256u + (unsigned)drop - t * (unsigned)hop : 0u;
            a[u] = ws[off];
            b[u] = xc[(long long)t * N + off];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (j < cnt[u]) acc[u] += a[u] * b[u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const unsigned s = s0 + u * 256u;
        if (s < out_len) y[(clip0 + c) * y_stride + s] = wss_is_norm ? acc[u] * w[u] : ((w[u] > tinyv) ? acc[u] / w[u] : acc[u]);
    }
}

template <class E> __global__ void transpose_kernel(const E* __restrict__ src, E* __restrict__ dst, long long rows, long long cols) {
    __shared__ E tile[32][33];
    const long long b = blockIdx.z;
    const long long r0 = (long long)blockIdx.y * 32, c0 = (long long)blockIdx.x * 32;
    const E* s = src + b * rows * cols;
    E* d = dst + b * rows * cols;
    for (int j = threadIdx.y; j < 32; j += 8) {
        const long long r = r0 + j, c = c0 + threadIdx.x;
        if (r < rows && c < cols) tile[j][threadIdx.x] = s[r * cols + c];
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += 8) {
        const long long c = c0 + j, r = r0 + threadIdx.x;
        if (r < rows && c < cols) d[c * rows + r] = tile[threadIdx.x][j];
    }
}

namespace {

}  // namespace

// Whole-signal rocFFT plans of the Fourier-domain resampler, one cache per (direction, precision, length), least recently used of
// kMaxResampleLengths evicted (signals of many different lengths must not accumulate plans and work buffers), and the two spectra.
constexpr size_t kMaxResampleLengths = 12;
struct ResampleFft {
    struct Entry {
        int type, dtype;
        long long n;
        std::unique_ptr<FftPlanCache> cache;
    };
    std::vector<Entry> entries;  // most recently used last
    Scratch spec_in, spec_out;
    Scratch time_in, time_out;  // padded clips / uncropped results of the band-limited form
    FftPlanCache order;  // cross-stream ordering of the two spectra (scratch_acquire / scratch_release)
    // the four buffers only ever grew (up to ~1 GB per pass each way), so one large call pinned ~2 GB of HBM for the context's lifetime.
    // A call that leaves more than kKeepBytes behind waits for its own work and gives the memory back (such a call ran for milliseconds anyway).
    // that wait + four hipFree (each a device-wide synchronisation) + the next call's re-allocation serialised every LOOP of large calls, and
    // inside a fork / join region (the constant-Q octave chain with the Fourier resamplers) it took the side stream's overlap away.  So: never inside a
    // fork / join region, and not while such calls follow each other closely (the previous one also ended oversize less than 100 ms ago) -- a lone large
    // call still gives its memory back at once; the last call of a loop leaves it to the next resample call on this context or to lra_ctx_destroy.
    static constexpr size_t kKeepBytes = 256u << 20;
    std::chrono::steady_clock::time_point last_oversize{};
    bool have_last_oversize = false;
    int trim(hipStream_t stream, bool in_fork_region) {
        if (spec_in.bytes + spec_out.bytes + time_in.bytes + time_out.bytes <= kKeepBytes) return LRA_OK;
        if (in_fork_region) return LRA_OK;
        const auto now = std::chrono::steady_clock::now();
        const bool in_loop = have_last_oversize && now - last_oversize < std::chrono::milliseconds(100);
        last_oversize = now;
        have_last_oversize = true;
        if (in_loop) return LRA_OK;
        LRA_HIP(hipStreamSynchronize(stream));
        for (Scratch* sc : {&spec_in, &spec_out, &time_in, &time_out}) {
            if (sc->p) (void)hipFree(sc->p);
            sc->p = nullptr;
            sc->bytes = 0;
        }
        return LRA_OK;
    }
    FftPlanCache* get(int type, int dtype, long long n) {
        for (size_t i = 0; i < entries.size(); ++i)
            if (entries[i].type == type && entries[i].dtype == dtype && entries[i].n == n) {
                Entry e = std::move(entries[i]);
                entries.erase(entries.begin() + (long)i);
                entries.push_back(std::move(e));
                return entries.back().cache.get();
            }
        if (entries.size() >= kMaxResampleLengths) {
            (void)hipDeviceSynchronize();  // the evicted plans may still have work in flight
            entries.erase(entries.begin());
        }
        entries.push_back(Entry{type, dtype, n, std::make_unique<FftPlanCache>()});
        return entries.back().cache.get();
    }
};

namespace {

int get_rocfft_plan(FftPlanCache& cache, lra_ctx* ctx, rocfft_transform_type type, int dtype, int n_fft, long long count, rocfft_plan* out) {
    rocfft_setup_once();
    rocfft_plan plan = nullptr;
    for (size_t i = 0; i < cache.plans.size(); ++i)
        if (cache.plans[i].first == count) {
            plan = cache.plans[i].second;
            cache.plans.erase(cache.plans.begin() + (long)i);
            break;
        }
    if (!plan) {
        size_t lengths[1] = {(size_t)n_fft};
        LRA_FFT(rocfft_plan_create(&plan, rocfft_placement_notinplace, type, dtype == LRA_F64 ? rocfft_precision_double : rocfft_precision_single, 1,
                                   lengths, (size_t)count, nullptr));
        if (cache.plans.size() >= kMaxFftPlans) {
            // the evicted plan may still have work in flight on the stream that used it last
            if (cache.last_use) (void)hipEventSynchronize(cache.last_use);
            rocfft_plan_destroy(cache.plans.front().second);
            cache.plans.erase(cache.plans.begin());
        }
    }
    cache.plans.emplace_back(count, plan);
    size_t wb = 0;
    LRA_FFT(rocfft_plan_get_work_buffer_size(plan, &wb));
    if (!cache.info) LRA_FFT(rocfft_execution_info_create(&cache.info));
    if (wb > cache.work_bytes) {
        if (cache.work) (void)hipFree(cache.work);  // hipFree synchronises with the device first
        cache.work = nullptr;
        cache.work_bytes = 0;
        LRA_HIP(hipMalloc(&cache.work, wb));
        cache.work_bytes = wb;
    }
    if (wb) LRA_FFT(rocfft_execution_info_set_work_buffer(cache.info, cache.work, cache.work_bytes));
    LRA_FFT(rocfft_execution_info_set_stream(cache.info, ctx->stream));
    *out = plan;
    return LRA_OK;
}

// `total` transforms of length n_fft, input stride in_stride / output stride out_stride (elements of in_elem / out_elem
// bytes), as full chunks of kFftChunk transforms + one remainder
int run_rocfft_chunked(FftPlanCache& cache, lra_ctx* ctx, rocfft_transform_type type, int dtype, int n_fft, long long total, char* in, size_t in_bytes_per_transform,
                       char* out, size_t out_bytes_per_transform) {
    for (long long t0 = 0; t0 < total;) {
        const long long cnt = total - t0 >= kFftChunk ? kFftChunk : total - t0;
        rocfft_plan plan;
        LRA_TRY(get_rocfft_plan(cache, ctx, type, dtype, n_fft, cnt, &plan));
        void* ib[1] = {in + (size_t)t0 * in_bytes_per_transform};
        void* ob[1] = {out + (size_t)t0 * out_bytes_per_transform};
        LRA_FFT(rocfft_execute(plan, ib, ob, cache.info));
        t0 += cnt;
    }
    return LRA_OK;
}

// scratch ordering across streams (see FftPlanCache): call before the first and after the last kernel of a general-path call
int scratch_acquire(FftPlanCache& cache, hipStream_t stream) {
    if (cache.last_use && cache.last_stream != stream) LRA_HIP(hipStreamWaitEvent(stream, cache.last_use, 0));
    return LRA_OK;
}
int scratch_release(FftPlanCache& cache, hipStream_t stream) {
    if (!cache.last_use) LRA_HIP(hipEventCreateWithFlags(&cache.last_use, hipEventDisableTiming));
    LRA_HIP(hipEventRecord(cache.last_use, stream));
    cache.last_stream = stream;
    return LRA_OK;
}

int power_mode_of(double power) { return power == 2.0 ? POW_TWO : (power == 1.0 ? POW_ONE : POW_GENERAL); }

// clips per pass of the general path so that the frame scratch stays <= ~4 GiB
long long general_clip_group(long long batch, long long frames_per_clip, int n_fft, size_t elem) {
    const double per_clip = (double)frames_per_clip * (double)n_fft * (double)elem;
    long long g = (long long)(4.0e9 / std::max(per_clip, 1.0));
    if (g < 1) g = 1;
    if (g > batch) g = batch;
    return g;
}

template <class T>
int stft_general(lra_stft_plan* p, const T* y, long long batch, long long n, long long y_stride, long long n_frames, cx<T>* D) {
    lra_ctx* ctx = p->ctx;
    const int N = p->n_fft, bins = N / 2 + 1;
    const long long group = general_clip_group(batch, n_frames, N, sizeof(T));
    LRA_TRY(p->frames.ensure((size_t)group * n_frames * N * sizeof(T)));
    for (long long c0 = 0; c0 < batch; c0 += group) {
        const long long clips = std::min(group, batch - c0);
        const long long total = clips * n_frames;
        const int chunks = (N + 255) / 256;
        hipLaunchKernelGGL(frame_window_kernel<T>, dim3((unsigned)(total * chunks)), dim3(256), 0, ctx->stream, y, y_stride, n, (int)n_frames, p->hop,
                           p->center ? N / 2 : 0, p->pad_mode, (const T*)p->d_win, N, c0, total, (T*)p->frames.p);
        LRA_HIP(hipGetLastError());
        LRA_TRY(run_rocfft_chunked(p->fft, ctx, rocfft_transform_type_real_forward, p->dtype, N, total, (char*)p->frames.p, (size_t)N * sizeof(T),
                                   (char*)(D + c0 * n_frames * bins), (size_t)bins * sizeof(cx<T>)));
    }
    return LRA_OK;
}

// times launch(0) and launch(4) (one warm-up, then two timed launches each) on the context's stream
template <class F> int autotune_variant(lra_ctx* ctx, F&& launch, int* tuned) {
    hipEvent_t e0, e1;
    LRA_HIP(hipEventCreate(&e0));
    LRA_HIP(hipEventCreate(&e1));
    float best = 0.f;
    int best_v = 0, rc = LRA_OK;
    const int cands[2] = {0, 4};
    for (int c = 0; c < 2 && rc == LRA_OK; ++c) {
        rc = launch(cands[c]);
        if (rc != LRA_OK) break;
        (void)hipEventRecord(e0, ctx->stream);
        rc = launch(cands[c]);
        if (rc == LRA_OK) rc = launch(cands[c]);
        (void)hipEventRecord(e1, ctx->stream);
        if (hipEventSynchronize(e1) != hipSuccess) { rc = fail(LRA_EHIP, "autotune: event synchronize failed"); break; }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        if (c == 0 || ms < best) { best = ms; best_v = cands[c]; }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc == LRA_OK) *tuned = best_v;
    return rc;
}

template <class T>
int stft_run(lra_stft_plan* p, int mode, const void* y, int64_t batch, int64_t n, int64_t y_stride, double power, lra_mel_plan* mel, void* out, int64_t row_pitch = 0) {
    LRA_BIND(p->ctx);
    int64_t n_frames = 0;
    LRA_TRY(lra_stft_num_frames(p, n, &n_frames));
    if (batch <= 0) return LRA_OK;
    if (!y || !out) return fail(LRA_EINVAL, "null data pointer");
    if (y_stride < n) return fail(LRA_EINVAL, "y_stride smaller than n");
    if (n_frames > 0x7fffffffLL / 4) return fail(LRA_EINVAL, "too many frames per clip");
    lra_ctx* ctx = p->ctx;
    const int bins = p->n_fft / 2 + 1;
    if (row_pitch <= 0) row_pitch = bins;
    if (row_pitch != bins && (!p->pow2 || row_pitch < bins || (mode != OUT_COMPLEX && mode != OUT_POWER)))
        return fail(LRA_EINVAL, "a row pitch other than n_bins is served by the fused power-of-two kernels only (complex / power results), and must be at least n_bins");
    if (mode == OUT_MEL) {
        if (!mel) return fail(LRA_EINVAL, "null mel plan");
        if (mel->n_bins != bins) return fail(LRA_EINVAL, "mel basis has " + std::to_string(mel->n_bins) + " bins, stft has " + std::to_string(bins));
        if (mel->dtype != p->dtype) return fail(LRA_EINVAL, "mel plan dtype differs from stft plan dtype");
    }
    // (powers of two in lra_mixed_sizes.h's forward list: the fused mel goes to the flat-index kernel further down, everything else stays here)
    // where it wins, measured on 256 x 30 s: n_fft 256 from 56 bands (80 bands at hop 64: 2.02 -> 1.28 ms; 48 bands 0.92 against 1.15: stays), n_fft 128 from 40
    // (64 bands at hop 32: 3.63 -> 2.06; 32 bands 1.51 against 1.71: stays)
    const bool pow2_mel_mixed = p->pow2 && mode == OUT_MEL && p->d_mtw && ctx->opt_mixed && ctx->opt_mixed_pow2_mel && row_pitch == bins && mel &&
                                mel->n_mels >= (p->n_fft >= 256 ? 56 : 40);
    if (p->pow2 && !pow2_mel_mixed) {
        StftLaunch<T> L;
        L.a = StftArgs<T>();
        L.a.y = (const T*)y;
        L.a.y_stride = y_stride;
        L.a.n = n;
        L.a.n_frames = (int)n_frames;
        L.a.row_pitch = row_pitch;
        L.a.hop = p->hop;
        L.a.pad = p->center ? p->n_fft / 2 : 0;
        L.a.pad_mode = p->pad_mode;
        L.a.win = (const T*)p->d_win;
        // measured on MI355X (bench.py --sweep): the two-wave-per-frame configuration wins when the mel
        // epilogue is fused in, the one-wave-per-frame configuration for the plain spectrum
        L.a.twr = (const cx<T>*)p->d_twr;
        L.out = out;
        L.a.power_mode = power_mode_of(power);
        L.a.power = (T)power;
        if (mel) {
            L.a.mel_c0 = mel->d_c0;
            L.a.mel_len = mel->d_len;
            L.a.mel_off = mel->d_off;
            L.a.mel_val = (const T*)mel->d_val;
            L.a.n_mels = mel->n_mels;
            L.a.mel_wAB = (const T*)mel->d_wAB;
            L.mel = mel;
        }
        L.a.nonfinite_flag = ctx->d_flag;
        L.mode = (mode == OUT_MEL && mel && mel->two_slope && !ctx->opt_generic_mel) ? OUT_MEL2 : mode;  // [sel:generic-mel-option]
        L.batch = batch;
        L.stream = ctx->stream;
        L.iters_opt = ctx->opt_stft_iters;
        L.n_cu = ctx->n_cu;
        L.mel_tile_opt = ctx->opt_mel_tile;
        L.lds_pad = ctx->opt_lds_pad;
        L.xcd_remap = ctx->opt_xcd_remap != 0;
        L.use_v2 = ctx->opt_v2 != 0;
        L.mel_pc = ctx->opt_mel_pc != 0;  // (which core: the variant chosen below)
        L.use_direct = ctx->opt_direct != 0;
        L.mel_runs = ctx->opt_mel_runs != 0;
        // Kernel variant (f32 n_fft = 2048 only): 0 = one wave per frame, 4 = two waves per frame.  Which one
        // is faster depends on the epilogue AND on the individual GPU (boxes of the same pool differ by +-10 %,
        // the one-wave variant being the more sensitive one), so unless the caller pinned a variant the first
        // large call of a plan times both on its own buffers (the kernels are idempotent) and keeps the winner.
        int variant = ctx->opt_variant >= 0 ? ctx->opt_variant : 0;
        auto launch = [&](int v) -> int {
            StftLaunch<T> Lv = L;
            Lv.a.tw = (const cx<T>*)p->d_tw[v];
            if (!dispatch_logm<T>(p->logm, v, Lv)) return fail(LRA_EINVAL, "unsupported power-of-two size");
            if (Lv.err != hipSuccess) return fail(LRA_EHIP, std::string("stft kernel launch: ") + hipGetErrorString(Lv.err));
            return LRA_OK;
        };
        // (the second-generation kernel replaces both tunings for the complex / power epilogues)
        bool v2_applies = false;
        if constexpr (sizeof(T) == 4)
            v2_applies = ctx->opt_v2 && (L.mode == OUT_COMPLEX || L.mode == OUT_POWER) && p->logm == 10 && v2_hop_divisor<typename CfgSel<float, 10, 0>::type>(p->hop) > 0;  // [sel:v2-applies]
        if (ctx->opt_variant < 0 && ctx->opt_autotune && sizeof(T) == 4 && p->logm == 10 && !v2_applies) {
            int& tuned = p->tuned_variant[L.mode & 3];
            if (tuned < 0 && batch * n_frames >= 65536) LRA_TRY(autotune_variant(ctx, launch, &tuned));  // [sel:autotune]
            if (tuned >= 0) variant = tuned;
        }
        bool pc_g = false;  // fused mel through the producer / consumer kernel on the radix 16-16-4 core (mel_pc = 2), where that kernel serves the bank and fits its register budget
        if constexpr (sizeof(T) == 4) {
            using C6 = typename CfgSel<float, 10, 6>::type;
            if (L.mode == OUT_MEL2 && ctx->opt_mel_pc == 2 && p->logm == 10 && mel && mel->melr2_ok && ctx->opt_mel_runs && ctx->opt_v2 && (ctx->opt_variant < 0 || ctx->opt_variant == 6))
                pc_g = pc_bank_ok<C6>(mel->n_mels, mel->melr2_pmax) && pc_fits_budget<C6>(v2_hop_divisor<C6>(p->hop), power_mode_of(power));
        }
        if ((v2_applies && (ctx->opt_v3 == 2 || (ctx->opt_v3 == 1 && L.mode == OUT_COMPLEX)) && (ctx->opt_variant < 0 || ctx->opt_variant == 6)) || pc_g) variant = 6;  // [sel:variant-fwd]
        else if (variant == 6) variant = 0;  // (the 16-16-4 form exists for the second-generation complex / power kernels and the producer / consumer mel kernel only)
        return launch(variant);
    }
    // listed non-power-of-two frame lengths: one fused launch (lra_mixed.h)
    if (p->d_mtw && ctx->opt_mixed) {
        mixed::Args<T> a = mixed::Args<T>();
        a.y = (const T*)y;
        a.y_stride = y_stride;
        a.n = n;
        a.n_frames = (int)n_frames;
        a.hop = p->hop;
        a.pad = p->center ? p->n_fft / 2 : 0;
        a.pad_mode = p->pad_mode;
        a.win = (const T*)(p->pow2 ? p->d_win_full : p->d_win);
        a.tw_m = (const mixed::cpx<T>*)p->d_mtw;
        a.tw_n = (const mixed::cpx<T>*)p->d_mtwn;
        a.power_mode = power_mode_of(power);
        a.power = (T)power;
        const int F = mixed::frames_per_group_of(p->n_fft, (int)sizeof(T));
        a.groups_per_clip = (int)((n_frames + F - 1) / F);
        int mm = mixed::MIXED_COMPLEX;
        if (mode == OUT_COMPLEX) {
            a.D = (mixed::cpx<T>*)out;
        } else if (mode == OUT_POWER) {
            a.S = (T*)out;
            mm = mixed::MIXED_POWER;
        } else {
            a.Mel = (T*)out;
            a.mel_c0 = mel->d_c0;
            a.mel_len = mel->d_len;
            a.mel_off = mel->d_off;
            a.mel_val = (const T*)mel->d_val;
            a.n_mels = mel->n_mels;
            a.mel_nnz = (ctx->opt_mixed != 2 && mixed::mel_lds_fits(mel->n_mels, mel->nnz)) ? mel->nnz : 0;  // band table staged in LDS (mixed = 2: cached reads, A/B)
            mm = mixed::MIXED_MEL;
        }
        hipError_t e;
        if constexpr (sizeof(T) == 8) e = mixed::launch_f64(p->n_fft, mm, a, batch, ctx->stream);
        else e = mixed::launch_f32(p->n_fft, mm, a, batch, ctx->stream);
        if (e != hipSuccess) return fail(LRA_EHIP, std::string("mixed-radix stft kernel launch: ") + hipGetErrorString(e));
        return LRA_OK;
    }
    // general path
    LRA_TRY(scratch_acquire(p->fft, ctx->stream));
    if (mode == OUT_COMPLEX) {
        LRA_TRY(stft_general<T>(p, (const T*)y, batch, n, y_stride, n_frames, (cx<T>*)out));
        return scratch_release(p->fft, ctx->stream);
    }
    // power / mel need the complex spectrum in scratch, one clip group at a time
    const long long group = general_clip_group(batch, n_frames, p->n_fft, sizeof(T));
    LRA_TRY(p->spec.ensure((size_t)group * n_frames * bins * sizeof(cx<T>) + (mode == OUT_MEL ? (size_t)group * n_frames * bins * sizeof(T) : 0)));
    cx<T>* Dtmp = (cx<T>*)p->spec.p;
    T* Stmp = (T*)((char*)p->spec.p + (size_t)group * n_frames * bins * sizeof(cx<T>));
    for (long long c0 = 0; c0 < batch; c0 += group) {
        const long long clips = std::min<long long>(group, batch - c0);
        LRA_TRY(stft_general<T>(p, (const T*)y + c0 * y_stride, clips, n, y_stride, n_frames, Dtmp));
        const long long count = clips * n_frames * bins;
        if (mode == OUT_POWER) {
            hipLaunchKernelGGL(power_kernel<T>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, Dtmp, (T*)out + c0 * n_frames * bins, count, power_mode_of(power), (T)power);
            LRA_HIP(hipGetLastError());
        } else {  // OUT_MEL: |D|^p transposed to [clip][bin][frame], then the banded product with lanes along the frames
            for (long long cz = 0; cz < clips; cz += 65535) {
                const long long nz = std::min<long long>(65535, clips - cz);
                hipLaunchKernelGGL(power_transpose_kernel<T>, dim3((unsigned)((bins + 31) / 32), (unsigned)((n_frames + 31) / 32), (unsigned)nz), dim3(32, 8), 0, ctx->stream,
                                   Dtmp + cz * n_frames * bins, Stmp + cz * n_frames * bins, (long long)n_frames, (long long)bins, power_mode_of(power), (T)power);
            }
            LRA_HIP(hipGetLastError());
            const long long tblocks = (n_frames + 255) / 256;
            hipLaunchKernelGGL(mel_apply_kernel<T>, dim3((unsigned)(tblocks * mel->n_mels * clips)), dim3(256), 0, ctx->stream, Stmp, n_frames * bins, (long long)n_frames,
                               1LL, n_frames, mel->n_mels, mel->d_c0, mel->d_len, mel->d_off, (const T*)mel->d_val,
                               (T*)out + c0 * mel->n_mels * n_frames);
            LRA_HIP(hipGetLastError());
        }
    }
    return scratch_release(p->fft, ctx->stream);
}

template <class T>
// `wss`: the window sum-square envelope of the output samples (wss_is_norm == 0, lra_istft_exec) or the normalisation factors made of it
// (1 / wss where wss > tiny, else 1: lra_istft_exec_norm, what the fused kernels consume).
int istft_run(lra_istft_plan* p, const void* D, int64_t batch, int64_t d_batch_stride, int64_t d_frame_stride, int64_t n_used, const void* wss, int wss_is_norm, void* y,
              int64_t out_len, int64_t y_stride) {
    LRA_BIND(p->ctx);
    lra_ctx* ctx = p->ctx;
    const int N = p->n_fft, bins = N / 2 + 1;
    if (batch <= 0 || out_len <= 0) return LRA_OK;
    if (!y || !wss) return fail(LRA_EINVAL, "null data pointer");
    if (y_stride < out_len) return fail(LRA_EINVAL, "y_stride smaller than out_len");
    // Samples [first, out_len) of every clip are zeroed here; everything below `first` is stored by the kernels themselves (the fused
    // kernel up to istft_written_end(), the gather kernel of the general path every sample), so the usual call clears nothing.  (Round 3
    // cleared the whole output first: 85 us and 677 MB of extra writes per 256 x 30 s call, 10.7 % of it.)
    auto zero_from = [&](long long first) -> int {
        if (first >= out_len) return LRA_OK;
        if (first < 0) first = 0;
        if (y_stride == out_len && first == 0) {
            LRA_HIP(hipMemsetAsync(y, 0, (size_t)batch * out_len * sizeof(T), ctx->stream));
        } else {
            LRA_HIP(hipMemset2DAsync((T*)y + first, (size_t)y_stride * sizeof(T), 0, (size_t)(out_len - first) * sizeof(T), (size_t)batch, ctx->stream));
        }
        return LRA_OK;
    };
    if (n_used <= 0) return zero_from(0);
    if (!D) return fail(LRA_EINVAL, "null spectrum pointer");
    if (d_frame_stride < bins) return fail(LRA_EINVAL, "d_frame_stride smaller than n_bins");
    const T tinyv = sizeof(T) == 8 ? (T)2.2250738585072014e-308 : (T)1.17549435e-38f;
    // listed non-power-of-two frame lengths -- and powers of two up to 1024 whose hop is not n_fft / {2, 4, 8, 16} (the register-tiled kernel
    // below serves those hops through its general overlap-add mode: measured slower) -- : one fused launch (lra_mixed.h, mixed_istft_kernel)
    auto run_mixed = [&](bool* done) -> int {
        *done = false;
        if (p->d_mtw && ctx->opt_mixed) {
            const int fmax = mixed::inv_frames_max_of(N, (int)sizeof(T));
            const int halo = (N + p->hop - 1) / p->hop - 1;
            // halo frames are recomputed by the neighbouring group: worth it while they are a third of the work at most; everything else takes the inverse transform alone
            // (mixed_irfft_kernel) + the gather kernel below, which beats both the recomputing kernel at larger LDS tiers and the rocFFT path (round 6: 480 / 120 2.84 ->
            // 1.62 ms, 800 / 200 2.77 -> 1.63, 1200 / 300 4.8 -> 2.25, 3200 / 800 4.75 -> 2.52)
            if (fmax - halo >= 1 && fmax - halo >= 2 * halo) {
                const void* nrm = wss;
                if (!wss_is_norm) {
                    LRA_TRY(p->norm.ensure((size_t)out_len * sizeof(T)));
                    hipLaunchKernelGGL(wss_to_norm_kernel<T>, dim3((unsigned)((out_len + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)wss, tinyv, (T*)p->norm.p, (long long)out_len);
                    LRA_HIP(hipGetLastError());
                    nrm = p->norm.p;
                }
                mixed::InvArgs<T> a = mixed::InvArgs<T>();
                a.D = (const mixed::cpx<T>*)D;
                a.d_batch_stride = d_batch_stride;
                a.d_frame_stride = d_frame_stride;
                a.n_used = (int)n_used;
                a.hop = p->hop;
                a.drop = p->center ? N / 2 : 0;
                a.win_scaled = (const T*)p->d_win_scaled;
                a.tw_m = (const mixed::cpx<T>*)p->d_mtw;
                a.tw_n = (const mixed::cpx<T>*)p->d_mtwn;
                a.norm = (const T*)nrm;
                a.y = (T*)y;
                a.y_stride = y_stride;
                a.out_len = out_len;
                a.halo = halo;
                a.group_hops = fmax - halo;
                a.groups_per_clip = (int)((n_used + a.group_hops - 1) / a.group_hops);
                hipError_t e;
                if constexpr (sizeof(T) == 8) e = mixed::launch_inv_f64(N, a, batch, ctx->stream);
                else e = mixed::launch_inv_f32(N, a, batch, ctx->stream);
                if (e != hipSuccess) return fail(LRA_EHIP, std::string("mixed-radix istft kernel launch: ") + hipGetErrorString(e));
                // the kernel stores every sample up to the last frame's end; beyond it (`length` past the frames' reach) the output is zero
                *done = true;
                return zero_from((n_used - 1) * (long long)p->hop + N - (p->center ? N / 2 : 0));
            }
        }
        return LRA_OK;
    };
    if (p->pow2 && ctx->opt_mixed_inv_pow2 && p->d_mtw && p->hop * 2 != N && p->hop * 4 != N && p->hop * 8 != N && p->hop * 16 != N && p->hop < N) {  // [sel:istft-mixed-pow2]
        bool done = false;
        LRA_TRY(run_mixed(&done));
        if (done) return LRA_OK;
    }
    if (p->pow2) {
        const void* nrm = wss;
        if (!wss_is_norm) {  // one tiny launch per call (out_len values); callers that keep the envelope around pass the factors themselves
            LRA_TRY(p->norm.ensure((size_t)out_len * sizeof(T)));
            hipLaunchKernelGGL(wss_to_norm_kernel<T>, dim3((unsigned)((out_len + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)wss, tinyv, (T*)p->norm.p, (long long)out_len);
            LRA_HIP(hipGetLastError());
            nrm = p->norm.p;
        }
        IstftLaunch<T> L;
        L.a = IstftArgs<T>();
        L.a.D = (const cx<T>*)D;
        L.a.d_batch_stride = d_batch_stride;
        L.a.d_frame_stride = d_frame_stride;
        L.a.n_used = (int)n_used;
        L.a.hop = p->hop;
        L.a.drop = p->center ? N / 2 : 0;
        L.a.win_scaled = (const T*)p->d_win_scaled;
        L.a.twr = (const cx<T>*)p->d_twr;
        L.a.wss = (const T*)nrm;
        L.a.tiny = tinyv;
        L.a.y = (T*)y;
        L.a.y_stride = y_stride;
        L.a.out_len = out_len;
        L.batch = batch;
        L.stream = ctx->stream;
        L.strip_frames = ctx->opt_istft_strip_groups > 0 ? ctx->opt_istft_strip_groups : 0;
        L.n_cu = ctx->n_cu;
        L.xcd_remap = ctx->opt_xcd_remap != 0;
        int variant = ctx->opt_variant >= 0 ? ctx->opt_variant : 0;  // see stft_run
        // f32 n_fft = 2048 with hop = n_fft / {2, 4, 8}: the ascending-radix configuration (variant 5), whose Hermitian step is
        // fused into the first pass, replaces both tunings
        bool fused_first_pass = false;
        if constexpr (sizeof(T) == 4)
            fused_first_pass = ctx->opt_v2 && ctx->opt_variant < 0 && p->logm == 10 && istft_rows_hc<typename CfgSel<float, 10, 5>::type>(p->hop) > 0;
        if (fused_first_pass) variant = ctx->opt_istft16 ? 7 : 5;  // 7: the same with 16-byte spectrum loads (radices 4, 16, 16)  // [sel:variant-inv]
        bool too_big = false;
        auto launch = [&](int v) -> int {
            IstftLaunch<T> Lv = L;
            Lv.a.tw = (const cx<T>*)p->d_tw[v];
            if (!dispatch_logm<T>(p->logm, v, Lv)) return fail(LRA_EINVAL, "unsupported power-of-two size");
            if (Lv.too_big) { too_big = true; return LRA_OK; }
            if (Lv.err != hipSuccess) return fail(LRA_EHIP, std::string("istft kernel launch: ") + hipGetErrorString(Lv.err));
            return LRA_OK;
        };
        if (ctx->opt_variant < 0 && ctx->opt_autotune && sizeof(T) == 4 && p->logm == 10 && !fused_first_pass) {
            int& tuned = p->tuned_variant[0];
            if (tuned < 0 && batch * n_used >= 65536) LRA_TRY(autotune_variant(ctx, launch, &tuned));
            if (tuned >= 0) variant = tuned;
        }
        LRA_TRY(launch(variant));
        if (!too_big) return zero_from(istft_written_end(N, p->hop, n_used, p->center ? N / 2 : 0));
    }
    if (!p->pow2) {
        bool done = false;
        LRA_TRY(run_mixed(&done));
        if (done) return LRA_OK;
    }
    // general path: pack -> rocFFT C2R -> gather overlap-add, one clip group at a time
    LRA_TRY(scratch_acquire(p->fft, ctx->stream));
    const long long group = general_clip_group(batch, n_used, N, sizeof(T));
    LRA_TRY(p->spec.ensure((size_t)group * n_used * bins * sizeof(cx<T>)));
    LRA_TRY(p->frames.ensure((size_t)group * n_used * N * sizeof(T)));
    for (long long c0 = 0; c0 < batch; c0 += group) {
        const long long clips = std::min<long long>(group, batch - c0);
        const long long total = clips * n_used;
        const int chunks = (bins + 255) / 256;
        if (!p->pow2 && p->d_mtw && ctx->opt_mixed && ctx->opt_mixed_irfft) {
            // listed mixed-radix lengths whose frames are too long for the fused gather kernel: the inverse real transform as ONE launch (lra_mixed.h, mixed_irfft_kernel)
            // instead of spec_pack + rocFFT C2R (round 6)
            mixed::IrArgs<T> ia = mixed::IrArgs<T>();
            ia.D = (const mixed::cpx<T>*)D + c0 * d_batch_stride;
            ia.d_batch_stride = d_batch_stride;
            ia.d_frame_stride = d_frame_stride;
            ia.n_used = (int)n_used;
            ia.tw_m = (const mixed::cpx<T>*)p->d_mtw;
            ia.tw_n = (const mixed::cpx<T>*)p->d_mtwn;
            ia.frames = (T*)p->frames.p;
            const int F = mixed::frames_per_group_of(N, (int)sizeof(T));
            ia.groups_per_clip = (int)((n_used + F - 1) / F);
            hipError_t e;
            if constexpr (sizeof(T) == 8) e = mixed::launch_irfft_f64(N, ia, clips, ctx->stream);
            else e = mixed::launch_irfft_f32(N, ia, clips, ctx->stream);
            if (e != hipSuccess) return fail(LRA_EHIP, std::string("mixed-radix inverse transform launch: ") + hipGetErrorString(e));
        } else {
        hipLaunchKernelGGL(spec_pack_kernel<T>, dim3((unsigned)(total * chunks)), dim3(256), 0, ctx->stream, (const cx<T>*)D, (long long)d_batch_stride,
                           (long long)d_frame_stride, (int)n_used, bins, (N % 2) == 0 ? 1 : 0, c0, total, (cx<T>*)p->spec.p);
        LRA_HIP(hipGetLastError());
        LRA_TRY(run_rocfft_chunked(p->fft, ctx, rocfft_transform_type_real_inverse, p->dtype, N, total, (char*)p->spec.p, (size_t)bins * sizeof(cx<T>),
                                   (char*)p->frames.p, (size_t)N * sizeof(T)));
        }
        const long long ochunks = (out_len + 255) / 256;
        const long long ochunks4 = (out_len + 1023) / 1024;
        if (ctx->opt_ola4 && out_len + (long long)N + 2048 < 0x7fffffffLL && n_used >= 1 && clips * ochunks4 < 0x7fffffffLL)
            hipLaunchKernelGGL(ola_gather4_kernel<T>, dim3((unsigned)(clips * ochunks4)), dim3(256), 0, ctx->stream, (const T*)p->frames.p, N, p->hop, (int)n_used,
                               p->center ? N / 2 : 0, (const T*)p->d_win_scaled, (const T*)wss, wss_is_norm, tinyv, c0, clips, (T*)y, (long long)y_stride, (unsigned)out_len,
                               (unsigned)ochunks4);
        else
            hipLaunchKernelGGL(ola_gather_kernel<T>, dim3((unsigned)(clips * ochunks)), dim3(256), 0, ctx->stream, (const T*)p->frames.p, N, p->hop, (int)n_used,
                               p->center ? N / 2 : 0, (const T*)p->d_win_scaled, (const T*)wss, wss_is_norm, tinyv, c0, clips, (T*)y, (long long)y_stride, (long long)out_len);
        LRA_HIP(hipGetLastError());
    }
    return scratch_release(p->fft, ctx->stream);
}

}  // namespace

// launch helpers of the decibel / MFCC entry points (lra_post.h)
namespace {
int post_chunks(long long batch, long long per_item, int n_cu) {
    // enough workgroups to fill the chip even for one big item, at least ~16 K elements each
    long long want = (8LL * n_cu + batch - 1) / (batch > 0 ? batch : 1);
    const long long most = (per_item + 16383) / 16384;
    if (want > most) want = most;
    return (int)(want < 1 ? 1 : want);
}
template <class T>
int to_db_run(lra_ctx* ctx, const void* x, void* out, long long batch, long long per_item, int amplitude, double amin, double ref_scalar, const void* ref_items, const void* item_max,
              int use_top_db, double top_db) {
    DbArgs<T> d;
    d.amin = (T)amin;
    d.ref_scalar = (T)ref_scalar;
    d.ref_items = (const T*)ref_items;
    d.item_max = use_top_db ? (const T*)item_max : nullptr;
    d.top_db = (T)top_db;
    const int chunks = post_chunks(batch, per_item, ctx->n_cu);
    const long long grid = batch * chunks;
    if (grid > 0x7fffffffLL) return fail(LRA_EINVAL, "too many items");
    if (amplitude) hipLaunchKernelGGL((to_db_kernel<T, true>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, (const T*)x, (T*)out, per_item, chunks, d);
    else hipLaunchKernelGGL((to_db_kernel<T, false>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, (const T*)x, (T*)out, per_item, chunks, d);
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}
template <class T, bool DB>
int dct_run(lra_ctx* ctx, const T* S, T* out, long long batch, int n_in, int n_out, long long n_frames, const T* C, const T* lift, const DbArgs<T>& d) {
    const long long tblocks = (n_frames + 255) / 256;
    const long long grid = tblocks * batch;
    if (grid > 0x7fffffffLL) return fail(LRA_EINVAL, "grid too large");
    // the basis arrives band-major, its coefficient axis padded with zeros to whole groups of 128 (lra_dct_exec's contract); every group is one launch
    const int ldc = (n_out + 127) / 128 * 128;  // the band-major basis [n_in][ldc] (lra_dct_exec's contract)
    for (int k0 = 0; k0 < n_out; k0 += 128) {
        const int rows = n_out - k0 < 128 ? n_out - k0 : 128;
        const T* Ck = C + k0;
        T* ok = out + (size_t)k0 * n_frames;
#define LRA_DCT(N) hipLaunchKernelGGL((dct_rows_kernel<T, N, DB>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, S, ok, n_frames, n_in, rows, n_out, Ck, ldc, lift + k0, d)
        if (rows <= 16) LRA_DCT(16);
        else if (rows <= 32) LRA_DCT(32);
        else if (rows <= 64) LRA_DCT(64);
        else LRA_DCT(128);
#undef LRA_DCT
        LRA_HIP(hipGetLastError());
    }
    return LRA_OK;
}
}  // namespace


// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
// ---- host-buffer entry point: chunked, overlapped H2D / kernel / D2H ---------------------------------------------------------
namespace {

// util.valid_audio's finite test (util/utils.py:305) on a span of IEEE words: exponent field all ones
template <class W, W MASK> bool span_has_nonfinite(const void* p, size_t bytes) {
    const W* w = (const W*)p;
    const size_t count = bytes / sizeof(W);
    W bad = 0;
    for (size_t i = 0; i < count; ++i) bad |= (W)((w[i] & MASK) == MASK);
    return bad != 0;
}

// rows x row_bytes between a strided and a packed buffer, split over a few host threads (one core copies ~10 GB/s, the
// link moves ~50).  scan_elem = 4 / 8: the copied samples (f32 / f64) are also tested for NaN / Inf while they are in
// cache; returns true when one was seen.
bool staged_copy(char* dst, size_t dst_stride, const char* src, size_t src_stride, size_t rows, size_t row_bytes, int threads, int scan_elem = 0) {
    const size_t total = rows * row_bytes;
    if (!total) return false;
    std::atomic<int> bad{0};
    auto span = [&bad, dst, dst_stride, src, src_stride, row_bytes, scan_elem](size_t lo, size_t hi) {
        size_t pos = lo;
        bool b = false;
        while (pos < hi) {
            const size_t r = pos / row_bytes, off = pos % row_bytes;
            const size_t len = std::min(row_bytes - off, hi - pos);
            char* d = dst + r * dst_stride + off;
            std::memcpy(d, src + r * src_stride + off, len);
            if (scan_elem == 4) b |= span_has_nonfinite<uint32_t, 0x7f800000u>(d, len);
            else if (scan_elem == 8) b |= span_has_nonfinite<uint64_t, 0x7ff0000000000000ull>(d, len);
            pos += len;
        }
        if (b) bad.store(1);
    };
    if (threads < 2 || total < (size_t)4 << 20) {
        span(0, total);
        return bad.load() != 0;
    }
    // byte spans (multiples of 8, so element boundaries are kept), not row ranges: one long row (a single clip) is shared too
    std::vector<std::thread> pool;
    const size_t per = (((total + threads - 1) / threads) + 7) & ~(size_t)7;
    for (int t = 0; t < threads; ++t) {
        const size_t lo = (size_t)t * per, hi = std::min(total, lo + per);
        if (lo >= hi) break;
        pool.emplace_back(span, lo, hi);
    }
    for (auto& th : pool) th.join();
    return bad.load() != 0;
}

int pipe_ensure(lra_ctx* ctx, size_t in_bytes, size_t out_bytes) {
    if (!ctx->pipe) {
        ctx->pipe = new HostPipe();
        HostPipe* hp = ctx->pipe;
        LRA_HIP(hipStreamCreateWithFlags(&hp->s_in, hipStreamNonBlocking));
        LRA_HIP(hipStreamCreateWithFlags(&hp->s_out, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            LRA_HIP(hipEventCreateWithFlags(&hp->ev_in[i], hipEventDisableTiming));
            LRA_HIP(hipEventCreateWithFlags(&hp->ev_comp[i], hipEventDisableTiming));
            LRA_HIP(hipEventCreateWithFlags(&hp->ev_out[i], hipEventDisableTiming));
        }
    }
    HostPipe* hp = ctx->pipe;
    if (in_bytes > hp->in_cap) {
        hp->release_buffers(true, false);
        for (int i = 0; i < 2; ++i) {
            LRA_HIP(hipHostMalloc(&hp->pin_in[i], in_bytes, hipHostMallocDefault));
            LRA_HIP(hipMalloc(&hp->dev_in[i], in_bytes));
        }
        hp->in_cap = in_bytes;
    }
    if (out_bytes > hp->out_cap) {
        hp->release_buffers(false, true);
        for (int i = 0; i < 2; ++i) {
            LRA_HIP(hipHostMalloc(&hp->pin_out[i], out_bytes, hipHostMallocDefault));
            LRA_HIP(hipMalloc(&hp->dev_out[i], out_bytes));
        }
        hp->out_cap = out_bytes;
    }
    return LRA_OK;
}

// The staged loop shared by the host-buffer entry points: `batch` items of in_item bytes (in_stride apart in the caller's
// buffer) go up, launch(dev_in, dev_out, first_item, n_items) runs on the compute stream, out_item bytes per item come down
// (out_stride apart).  Slot s = stage & 1; events order slot reuse; the host thread copies stage c in while stage c - 1's
// kernel / download run, then hands stage c - 1 to the caller.
template <class Launch>
int host_pipeline(lra_ctx* ctx, int64_t batch, size_t in_item, size_t in_stride, size_t out_item, size_t out_stride, const char* in, char* out, int scan_elem, bool* bad_out, Launch&& launch) {
    // items per stage: ~pipe_chunk_mb of traffic, at least one item, at least two stages when there are two items
    int64_t per = (int64_t)(((size_t)ctx->opt_pipe_chunk_mb << 20) / (in_item + out_item));
    per = std::max<int64_t>(1, std::min<int64_t>(per, (batch + 1) / 2));
    LRA_TRY(pipe_ensure(ctx, (size_t)per * in_item, (size_t)per * out_item));
    HostPipe* hp = ctx->pipe;
    hipStream_t compute = ctx->stream;
    const int64_t chunks = (batch + per - 1) / per;
    auto drain = [&](int64_t c) -> int {  // pinned_out[slot of c] -> the caller's buffer
        const int s = (int)(c & 1);
        const int64_t b0 = c * per, nb = std::min(per, batch - b0);
        LRA_HIP(hipEventSynchronize(hp->ev_out[s]));
        staged_copy(out + (size_t)b0 * out_stride, out_stride, (const char*)hp->pin_out[s], out_item, (size_t)nb, out_item, ctx->opt_pipe_threads);
        return LRA_OK;
    };
    auto body = [&]() -> int {
        bool bad = false;
        for (int64_t c = 0; c < chunks; ++c) {
            const int s = (int)(c & 1);
            const int64_t b0 = c * per, nb = std::min(per, batch - b0);
            // slot s: its previous upload (stage c - 2) must have left the pinned buffer before the host overwrites it
            if (c >= 2) LRA_HIP(hipEventSynchronize(hp->ev_in[s]));
            if (staged_copy((char*)hp->pin_in[s], in_item, in + (size_t)b0 * in_stride, in_stride, (size_t)nb, in_item, ctx->opt_pipe_threads, scan_elem)) bad = true;
            if (c >= 2) LRA_HIP(hipStreamWaitEvent(hp->s_in, hp->ev_comp[s], 0));  // dev_in[s] is still read by stage c - 2's kernel
            LRA_HIP(hipMemcpyAsync(hp->dev_in[s], hp->pin_in[s], (size_t)nb * in_item, hipMemcpyHostToDevice, hp->s_in));
            LRA_HIP(hipEventRecord(hp->ev_in[s], hp->s_in));
            LRA_HIP(hipStreamWaitEvent(compute, hp->ev_in[s], 0));
            if (c >= 2) LRA_HIP(hipStreamWaitEvent(compute, hp->ev_out[s], 0));  // dev_out[s] still being downloaded (stage c - 2)
            LRA_TRY(launch(hp->dev_in[s], hp->dev_out[s], b0, nb));
            LRA_HIP(hipEventRecord(hp->ev_comp[s], compute));
            // this stage's download is queued BEFORE the previous stage is handed to the caller (round 6): it fills the other pinned slot while the host threads
            // empty that one -- queued after the hand-over, download and host copy took turns (64 x 30 s stft: 20.7 ms = 13.5 of download + 8 of host copy)
            LRA_HIP(hipStreamWaitEvent(hp->s_out, hp->ev_comp[s], 0));
            LRA_HIP(hipMemcpyAsync(hp->pin_out[s], hp->dev_out[s], (size_t)nb * out_item, hipMemcpyDeviceToHost, hp->s_out));
            LRA_HIP(hipEventRecord(hp->ev_out[s], hp->s_out));
            // the previous stage's download (slot 1 - s) has been running meanwhile: hand it to the caller before the next stage reuses its pinned slot
            if (c >= 1) LRA_TRY(drain(c - 1));
        }
        LRA_TRY(drain(chunks - 1));
        if (bad_out) *bad_out = bad;
        return LRA_OK;
    };
    const int rc = body();
    if (rc != LRA_OK) {  // leave no work in flight on buffers the next call reuses
        (void)hipStreamSynchronize(hp->s_in);
        (void)hipStreamSynchronize(compute);
        (void)hipStreamSynchronize(hp->s_out);
    }
    // A stage is at least one whole item, so one very long clip (an hour of audio: 0.3 GB in, 2.5 GB of spectrum out) sizes the
    // two pinned + two device slots far beyond pipe_chunk_mb.  Such slots do not outlive the call: only staging of up to four
    // nominal stages per direction persists in the context (what a streaming caller reuses block after block).
    const size_t keep_cap = (size_t)4 * ((size_t)ctx->opt_pipe_chunk_mb << 20);
    if (hp->in_cap > keep_cap || hp->out_cap > keep_cap) {
        (void)hipStreamSynchronize(hp->s_in);
        (void)hipStreamSynchronize(compute);
        (void)hipStreamSynchronize(hp->s_out);
        hp->release_buffers(hp->in_cap > keep_cap, hp->out_cap > keep_cap);
    }
    return rc;
}

}  // namespace

// ---- RCCL, bound at run time (the library does not link it: single-GPU users never load it) --------------------------------
struct lra_comm {
    lra_ctx* ctx = nullptr;
    void* nccl = nullptr;  // ncclComm_t
    int rank = 0, n_ranks = 1;
};

namespace {

struct RcclApi {
    struct Id { char b[128]; };  // ncclUniqueId (NCCL_UNIQUE_ID_BYTES = 128), passed by value
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, Id, int) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;  // (optional: lra_comm_allgatherv)
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};

RcclApi* rccl_api() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        // a copy the process has already loaded (PyTorch bundles its own) wins: two RCCLs in one process do not share state
        for (const char* name : {"librccl.so", "librccl.so.1"}) {
            api.lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
            if (api.lib) break;
        }
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            if (api.lib) break;
            api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        }
        if (!api.lib) return;
        api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.lib, "ncclGetUniqueId");
        api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.lib, "ncclCommInitRank");
        api.AllGather = (decltype(api.AllGather))dlsym(api.lib, "ncclAllGather");
        api.Broadcast = (decltype(api.Broadcast))dlsym(api.lib, "ncclBroadcast");
        api.GroupStart = (decltype(api.GroupStart))dlsym(api.lib, "ncclGroupStart");
        api.GroupEnd = (decltype(api.GroupEnd))dlsym(api.lib, "ncclGroupEnd");
        api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.lib, "ncclCommDestroy");
        api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.lib, "ncclGetErrorString");
    });
    return (api.lib && api.GetUniqueId && api.CommInitRank && api.AllGather && api.CommDestroy) ? &api : nullptr;
}

int rccl_fail(RcclApi* api, const char* what, int rc) {
    return fail(LRA_EHIP, std::string(what) + ": " + (api && api->GetErrorString ? api->GetErrorString(rc) : "RCCL error") + " (" + std::to_string(rc) + ")");
}

}  // namespace

namespace {
template <class T> void hpss_launch(lra_ctx* ctx, const void* mag, const void* D, void* out_h, void* out_p, const HpssArgs& a, unsigned grid) {
    const HpssPlan plan = hpss_plan(a, (int)sizeof(T));
    // a thread per 4 x 4 tile, neighbouring windows sharing one sorted core (hpss_tile_kernel)
    const unsigned tgrid = (unsigned)((hpss_tiles(a) + 255) / 256);
    if (plan.tile_slots == 32 && plan.fixed_win && ctx->opt_hpss_tile) {
        hipLaunchKernelGGL((hpss_tile_kernel<T, 32, kHpssFixedWin>), dim3(tgrid), dim3(256), 0, ctx->stream, (const T*)mag, (const HpssCplx<T>*)D, out_h, out_p, a);
        return;
    }
    if (plan.tile_slots == 32 && ctx->opt_hpss_tile) {
        hipLaunchKernelGGL((hpss_tile_kernel<T, 32, 0>), dim3(tgrid), dim3(256), 0, ctx->stream, (const T*)mag, (const HpssCplx<T>*)D, out_h, out_p, a);
        return;
    }
    if constexpr (sizeof(T) == 4) {
        if (plan.tile_slots == 64 && ctx->opt_hpss_tile) {
            hipLaunchKernelGGL((hpss_tile_kernel<T, 64, 0>), dim3(tgrid), dim3(256), 0, ctx->stream, (const T*)mag, (const HpssCplx<T>*)D, out_h, out_p, a);
            return;
        }
    }
    if (plan.element_slots == 32) {
        hipLaunchKernelGGL((hpss_kernel<T, 32>), dim3(grid), dim3(256), 0, ctx->stream, (const T*)mag, (const HpssCplx<T>*)D, out_h, out_p, a);
        return;
    }
    if constexpr (sizeof(T) == 4) {
        if (plan.element_slots == 64) {
            hipLaunchKernelGGL((hpss_kernel<T, 64>), dim3(grid), dim3(256), 0, ctx->stream, (const T*)mag, (const HpssCplx<T>*)D, out_h, out_p, a);
            return;
        }
    }
    hipLaunchKernelGGL((hpss_kernel<T, 0>), dim3(grid), dim3(256), 0, ctx->stream, (const T*)mag, (const HpssCplx<T>*)D, out_h, out_p, a);
}
}  // namespace

extern "C" {

const char* lra_last_error(void) { return g_err.c_str(); }
const char* lra_version(void) { return "librosa_amd 0.1 (gfx950)"; }

int lra_device_count(int* count) {
    if (!count) return fail(LRA_EINVAL, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(LRA_ENODEV, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = n;
    return LRA_OK;
}

int lra_ctx_create(int device, lra_ctx** out) {
    if (!out) return fail(LRA_EINVAL, "null out");
    *out = nullptr;
    int n = 0;
    if (lra_device_count(&n) != LRA_OK || n <= 0) return fail(LRA_ENODEV, "no HIP device available: librosa_amd has no CPU fallback");
    if (device < 0 || device >= n) return fail(LRA_EINVAL, "device index out of range");
    DeviceGuard device_guard__(device);
    if (device_guard__.err != hipSuccess) return fail(LRA_EHIP, std::string("selecting device: ") + hipGetErrorString(device_guard__.err));
    hipDeviceProp_t prop;
    LRA_HIP(hipGetDeviceProperties(&prop, device));
    lra_ctx* c = new lra_ctx();
    c->device = device;
    c->n_cu = prop.multiProcessorCount;
    c->name = std::string(prop.name) + " (" + prop.gcnArchName + ")";
    hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(LRA_EHIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    c->stream = c->own_stream;
    e = hipMalloc((void**)&c->d_flag, sizeof(unsigned int));
    if (e == hipSuccess) e = hipMemset(c->d_flag, 0, sizeof(unsigned int));
    if (e != hipSuccess) {
        (void)hipStreamDestroy(c->own_stream);
        delete c;
        return fail(LRA_EHIP, std::string("flag allocation: ") + hipGetErrorString(e));
    }
    *out = c;
    // LRA_CTX_OPTIONS="key=value,key=value": options applied to every context at creation (whole-suite runs with a kernel form switched on or off)
    if (const char* env = std::getenv("LRA_CTX_OPTIONS")) {
        std::string text(env);
        size_t pos = 0;
        while (pos < text.size()) {
            size_t end = text.find(',', pos);
            if (end == std::string::npos) end = text.size();
            const std::string kv = text.substr(pos, end - pos);
            pos = end + 1;
            if (kv.empty()) continue;
            const size_t eq = kv.find('=');
            int rc = eq == std::string::npos ? fail(LRA_EINVAL, "LRA_CTX_OPTIONS: expected key=value, got " + kv) : lra_ctx_set_option(c, kv.substr(0, eq).c_str(), std::atoi(kv.c_str() + eq + 1));
            if (rc != LRA_OK) {
                *out = nullptr;
                lra_ctx_destroy(c);
                return rc;
            }
        }
    }
    return LRA_OK;
}

namespace {
void placed_release(lra_ctx* ctx, void* ptr, lra_ctx::PlacedAlloc& pa);  // (defined with lra_malloc_placed below)
}

void lra_ctx_destroy(lra_ctx* ctx) {
    if (!ctx) return;
    DeviceGuard device_guard__(ctx->device);
    delete ctx->pipe;
    delete ctx->rs_fft;
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    if (ctx->side_stream) (void)hipStreamDestroy(ctx->side_stream);
    for (int i = 0; i < lra_ctx::kForkRing; ++i) {
        if (ctx->fork_event[i]) (void)hipEventDestroy(ctx->fork_event[i]);
        if (ctx->side_passed[i]) (void)hipEventDestroy(ctx->side_passed[i]);
    }
    for (int i = 0; i < lra_ctx::kJoinRing; ++i) {
        if (ctx->join_event[i]) (void)hipEventDestroy(ctx->join_event[i]);
        if (ctx->main_passed[i]) (void)hipEventDestroy(ctx->main_passed[i]);
    }
    if (ctx->d_flag) (void)hipFree(ctx->d_flag);
    if (!ctx->placed.empty()) (void)hipDeviceSynchronize();
    {
        std::map<void*, lra_ctx::PlacedAlloc> live;
        { std::lock_guard<std::mutex> lk(ctx->placed_mu); live.swap(ctx->placed); }
        for (auto& kv : live) placed_release(ctx, kv.first, kv.second);
        for (auto& r : ctx->placed_retired) (void)hipMemAddressFree(r.first, r.second);   // nothing of this context is mapped any more
        ctx->placed_retired.clear();
    }
    for (auto& kv : ctx->cqt_tw) {
        if (kv.second.first) (void)hipFree(kv.second.first);
        if (kv.second.second) (void)hipFree(kv.second.second);
    }
    delete ctx;
}

int lra_ctx_set_stream(lra_ctx* ctx, void* hip_stream) {
    if (!ctx) return fail(LRA_EINVAL, "null context");
    ctx->stream = (hipStream_t)hip_stream;  // NULL is HIP's default (null) stream, a valid choice
    ctx->on_side = ctx->side_used = false;
    return LRA_OK;
}

int lra_ctx_use_own_stream(lra_ctx* ctx) {
    if (!ctx) return fail(LRA_EINVAL, "null context");
    ctx->stream = ctx->own_stream;
    ctx->on_side = ctx->side_used = false;
    return LRA_OK;
}

int lra_ctx_side(lra_ctx* ctx, int mode) {
    LRA_BIND(ctx);
    if (mode == LRA_SIDE_FORK) {
        if (ctx->on_side) return fail(LRA_EINVAL, "lra_ctx_side: already on the side stream");
        if (!ctx->side_stream) {
            // the side stream carries work that runs BESIDE a dependent chain on the caller's stream (octave transforms beside the halvings): lowest
            // priority, so that the chain's short kernels are dispatched ahead of it
            int least = 0, greatest = 0;
            if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest)
                LRA_HIP(hipStreamCreateWithPriority(&ctx->side_stream, hipStreamNonBlocking, least));
            else
                LRA_HIP(hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking));
        }
        const int slot = ctx->fork_next;
        ctx->fork_next = (slot + 1) % lra_ctx::kForkRing;
        if (!ctx->fork_event[slot]) LRA_HIP(hipEventCreateWithFlags(&ctx->fork_event[slot], hipEventDisableTiming));
        if (!ctx->side_passed[slot]) LRA_HIP(hipEventCreateWithFlags(&ctx->side_passed[slot], hipEventDisableTiming));
        if (ctx->fork_used[slot]) LRA_HIP(hipEventSynchronize(ctx->side_passed[slot]));  // the side stream is past its wait on this slot's previous record
        LRA_HIP(hipEventRecord(ctx->fork_event[slot], ctx->stream));
        LRA_HIP(hipStreamWaitEvent(ctx->side_stream, ctx->fork_event[slot], 0));
        LRA_HIP(hipEventRecord(ctx->side_passed[slot], ctx->side_stream));
        ctx->fork_used[slot] = true;
        ctx->side_main = ctx->stream;
        ctx->stream = ctx->side_stream;
        ctx->on_side = ctx->side_used = true;
        return LRA_OK;
    }
    if (mode == LRA_SIDE_BACK) {
        if (!ctx->on_side) return fail(LRA_EINVAL, "lra_ctx_side: not on the side stream");
        ctx->stream = ctx->side_main;
        ctx->on_side = false;
        return LRA_OK;
    }
    if (mode == LRA_SIDE_END && ctx->on_side) {  // wherever the caller is (error paths): back, then join
        ctx->stream = ctx->side_main;
        ctx->on_side = false;
    }
    if (mode == LRA_SIDE_JOIN || mode == LRA_SIDE_END) {
        if (ctx->on_side) return fail(LRA_EINVAL, "lra_ctx_side: join from the main stream (LRA_SIDE_BACK first)");
        if (!ctx->side_used) return LRA_OK;
        const int js = ctx->join_next;
        ctx->join_next = (js + 1) % lra_ctx::kJoinRing;
        if (!ctx->join_event[js]) LRA_HIP(hipEventCreateWithFlags(&ctx->join_event[js], hipEventDisableTiming));
        if (!ctx->main_passed[js]) LRA_HIP(hipEventCreateWithFlags(&ctx->main_passed[js], hipEventDisableTiming));
        if (ctx->join_used[js]) LRA_HIP(hipEventSynchronize(ctx->main_passed[js]));  // the main stream is past its wait on this slot's previous record
        LRA_HIP(hipEventRecord(ctx->join_event[js], ctx->side_stream));
        LRA_HIP(hipStreamWaitEvent(ctx->stream, ctx->join_event[js], 0));
        LRA_HIP(hipEventRecord(ctx->main_passed[js], ctx->stream));
        ctx->join_used[js] = true;
        ctx->side_used = false;
        return LRA_OK;
    }
    return fail(LRA_EINVAL, "lra_ctx_side: mode must be LRA_SIDE_FORK, LRA_SIDE_BACK, LRA_SIDE_JOIN or LRA_SIDE_END");
}

int lra_ctx_sync(lra_ctx* ctx) {
    LRA_BIND(ctx);
    LRA_HIP(hipStreamSynchronize(ctx->stream));
    return LRA_OK;
}

int lra_ctx_set_option(lra_ctx* ctx, const char* key, int value) {
    if (!ctx || !key) return fail(LRA_EINVAL, "null argument");
    if (!std::strcmp(key, "stft_iters")) ctx->opt_stft_iters = value;
    else if (!std::strcmp(key, "istft_strip_groups")) ctx->opt_istft_strip_groups = value;
    else if (!std::strcmp(key, "mel_tile")) ctx->opt_mel_tile = value;
    else if (!std::strcmp(key, "ablate")) (void)value;  // retired development knob, accepted and ignored
    else if (!std::strcmp(key, "generic_mel")) ctx->opt_generic_mel = value;
    else if (!std::strcmp(key, "pipe_chunk_mb")) ctx->opt_pipe_chunk_mb = value > 0 ? value : 128;
    else if (!std::strcmp(key, "pipe_threads")) ctx->opt_pipe_threads = value > 0 ? value : 1;
    else if (!std::strcmp(key, "lds_pad")) ctx->opt_lds_pad = value;
    else if (!std::strcmp(key, "xcd_remap")) ctx->opt_xcd_remap = value != 0;
    else if (!std::strcmp(key, "v2")) ctx->opt_v2 = value != 0;
    else if (!std::strcmp(key, "mel_pc")) ctx->opt_mel_pc = (value == 1 || value == 2) ? value : 0;  // 1: on the radix 16-8-8 core, 2: on the radix 16-16-4 core
    else if (!std::strcmp(key, "istft16")) ctx->opt_istft16 = value != 0;
    else if (!std::strcmp(key, "placement_retry")) ctx->opt_placement_retry = value < 0 ? 0 : (value > 8 ? 8 : value);
    else if (!std::strcmp(key, "v3")) ctx->opt_v3 = (value == 1 || value == 2) ? value : 0;
    else if (!std::strcmp(key, "cqt_merge")) ctx->opt_cqt_merge = value < 0 ? 0 : (value > 2 ? 2 : (int)value);
    else if (!std::strcmp(key, "mel_many")) ctx->opt_mel_many = value != 0;
    else if (!std::strcmp(key, "direct")) ctx->opt_direct = value != 0;
    else if (!std::strcmp(key, "mixed")) ctx->opt_mixed = value == 2 ? 2 : (value != 0);
    else if (!std::strcmp(key, "hpss_tile")) ctx->opt_hpss_tile = value != 0;
    else if (!std::strcmp(key, "mixed_pow2_mel")) ctx->opt_mixed_pow2_mel = value != 0;
    else if (!std::strcmp(key, "ola4")) ctx->opt_ola4 = value != 0;
    else if (!std::strcmp(key, "mixed_irfft")) ctx->opt_mixed_irfft = value != 0;
    else if (!std::strcmp(key, "mixed_inv_pow2")) ctx->opt_mixed_inv_pow2 = value != 0;
    else if (!std::strcmp(key, "autotune")) ctx->opt_autotune = value != 0;
    else if (!std::strcmp(key, "mel_runs")) ctx->opt_mel_runs = value != 0;
    else if (!std::strcmp(key, "variant")) ctx->opt_variant = (value >= 0 && value < kNumVariants) ? value : -1;
    else return fail(LRA_EINVAL, std::string("unknown option ") + key);
    return LRA_OK;
}

int lra_ctx_nonfinite_reset(lra_ctx* ctx) {
    LRA_BIND(ctx);
    LRA_HIP(hipMemsetAsync(ctx->d_flag, 0, sizeof(unsigned int), ctx->stream));
    return LRA_OK;
}

int lra_ctx_nonfinite_read(lra_ctx* ctx, int* flag) {
    LRA_BIND(ctx);
    if (!flag) return fail(LRA_EINVAL, "null flag");
    unsigned int h = 0;
    LRA_HIP(hipMemcpyAsync(&h, ctx->d_flag, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    LRA_HIP(hipStreamSynchronize(ctx->stream));
    if (h & 2u) {  // a wave of the producer / consumer mel kernel gave up waiting for its partner (lra_kernels_pc.h, pc_wait): the result is not to be trusted
        (void)hipMemsetAsync(ctx->d_flag, 0, sizeof(unsigned int), ctx->stream);
        return fail(LRA_EHIP, "fused mel kernel: a producer / consumer hand-over timed out (results invalid); ctx option mel_pc = 0 selects the one-wave kernel");
    }
    *flag = (int)(h & 1u);
    return LRA_OK;
}

int lra_ctx_device_name(lra_ctx* ctx, char* buf, size_t buflen) {
    if (!ctx || !buf || !buflen) return fail(LRA_EINVAL, "null argument");
    std::snprintf(buf, buflen, "%s, %d CUs", ctx->name.c_str(), ctx->n_cu);
    return LRA_OK;
}

int lra_malloc(lra_ctx* ctx, size_t bytes, void** dptr) {
    LRA_BIND(ctx);
    if (!dptr) return fail(LRA_EINVAL, "null dptr");
    *dptr = nullptr;
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 16);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? LRA_ENOMEM : LRA_EHIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    return LRA_OK;
}

int lra_free(lra_ctx* ctx, void* dptr) {
    LRA_BIND(ctx);
    if (dptr) LRA_HIP(hipFree(dptr));
    return LRA_OK;
}

// ---- placement-aware allocation of large result buffers (round 6) ----------------------------------------------------------------
// profiles/r05_pitch.md: WHERE a 2.7 GB spectrum lands moves the store-bound transform between 0.63 and 0.75 ms on some boxes, nothing in user space
// steers it, but buffers built from 32-128 MiB physical handles created and mapped in order hit the fast levels far more often than one hipMalloc, and
// the bare write stream of the kernel reproduces the kernel's level.  So: build up to `tries` candidates that way (all alive at once -- a freed candidate's
// pages would come straight back), time the write stream on each, keep the best, release the others.  Early exits keep boxes without the lottery cheap: two
// candidates within 1.5 % of each other, or a candidate within 1.5 % of the best rate this context has ever seen, end the search.
namespace {
// (the kernels' geometry: an item -- a clip's frames -- is cut into strips of `strip` consecutive rows, the last one shorter, one wave per strip, workgroup b -> strip
//  (b mod 8) chunk + b / 8 as xcd_block does; which strips are written at the same time is what the placement levels are about, so the probe cuts the same way)
__global__ __launch_bounds__(64) void placed_probe_kernel(char* __restrict__ out, long long rows, int row_bytes, long long rows_per_item, int strip, int strips_per_item, int xcd_chunk) {
    typedef float f2p __attribute__((ext_vector_type(2)));
    extern __shared__ char placed_probe_pad[];  // (sized by the launch so that twelve waves share a CU, the forward kernel's residency)
    const int lane = threadIdx.x;
    long long b = blockIdx.x;
    if (xcd_chunk > 0) b = (b % 8) * (long long)xcd_chunk + b / 8;
    const long long item = b / strips_per_item, part = b % strips_per_item;
    const long long first = item * rows_per_item + part * strip;
    if (first >= rows || part * strip >= rows_per_item) return;
    const long long last = (item + 1) * rows_per_item < rows ? (item + 1) * rows_per_item : rows;
    const int pieces = row_bytes / 512;  // wave-wide instructions of 8 bytes per lane
    f2p v = {(float)lane, (float)b};
    for (int it = 0; it < strip && first + it < last; ++it) {
        f2p* rp = reinterpret_cast<f2p*>(out + (first + it) * (long long)row_bytes);
        for (int i = 0; i < pieces; ++i) rp[i * 64 + lane] = v;
        const int rest = (row_bytes - pieces * 512) / 8;
        if (lane < rest) rp[pieces * 64 + lane] = v;
        v.x += 1.0f;
    }
}

int placed_create(lra_ctx* ctx, size_t bytes, size_t chunk, void** ptr_out, lra_ctx::PlacedAlloc* pa) {
    const int device = ctx->device;
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = device;
    size_t gran = 0;
    LRA_HIP(hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended));
    if (gran == 0) gran = 2u << 20;
    chunk = (chunk + gran - 1) / gran * gran;
    const size_t padded = (bytes + chunk - 1) / chunk * chunk;
    {
        std::lock_guard<std::mutex> lk(ctx->placed_mu);
        if (ctx->placed_va_spent + padded > lra_ctx::kPlacedVaBudget) return fail(LRA_ENOMEM, "lra_malloc_placed: this context's address-space budget for placed buffers is spent (ranges are never re-used: see lra_ctx)");
        ctx->placed_va_spent += padded;
    }
    void* ptr = nullptr;
    hipError_t e = hipMemAddressReserve(&ptr, padded, 0, nullptr, 0);
    if (e != hipSuccess) return fail(LRA_EHIP, std::string("hipMemAddressReserve: ") + hipGetErrorString(e));
    pa->padded = padded;
    auto undo = [&]() {
        for (size_t i = 0; i < pa->handles.size(); ++i) {
            (void)hipMemUnmap((char*)ptr + i * chunk, chunk);
            (void)hipMemRelease(pa->handles[i]);
        }
        pa->handles.clear();
        std::lock_guard<std::mutex> lk(ctx->placed_mu);
        ctx->placed_retired.push_back({ptr, padded});  // (never hipMemAddressFree while the context lives)
    };
    for (size_t off = 0; off < padded; off += chunk) {
        hipMemGenericAllocationHandle_t h;
        e = hipMemCreate(&h, chunk, &prop, 0);
        if (e == hipSuccess) {
            e = hipMemMap((char*)ptr + off, chunk, 0, h, 0);
            if (e != hipSuccess) (void)hipMemRelease(h);
        }
        if (e != hipSuccess) {
            undo();
            return fail(e == hipErrorOutOfMemory ? LRA_ENOMEM : LRA_EHIP, std::string("hipMemCreate / hipMemMap: ") + hipGetErrorString(e));
        }
        pa->handles.push_back(h);
    }
    hipMemAccessDesc acc = {};
    acc.location.type = hipMemLocationTypeDevice;
    acc.location.id = device;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    e = hipMemSetAccess(ptr, padded, &acc, 1);
    if (e != hipSuccess) {
        undo();
        return fail(LRA_EHIP, std::string("hipMemSetAccess: ") + hipGetErrorString(e));
    }
    *ptr_out = ptr;
    return LRA_OK;
}

// physical memory back to the device; the (now empty) address range stays reserved and is never used again (see lra_ctx::placed_retired)
void placed_release(lra_ctx* ctx, void* ptr, lra_ctx::PlacedAlloc& pa) {
    if (!ptr) return;
    if (pa.plain) {
        (void)hipFree(ptr);
        return;
    }
    const size_t chunk = pa.handles.empty() ? pa.padded : pa.padded / pa.handles.size();
    for (size_t i = 0; i < pa.handles.size(); ++i) {
        (void)hipMemUnmap((char*)ptr + i * chunk, chunk);
        (void)hipMemRelease(pa.handles[i]);
    }
    pa.handles.clear();
    std::lock_guard<std::mutex> lk(ctx->placed_mu);
    ctx->placed_retired.push_back({ptr, pa.padded});
}

int placed_probe_ms(lra_ctx* ctx, void* ptr, size_t bytes, int row_bytes, long long rows_per_item, float* ms) {
    const long long rows = (long long)(bytes / (size_t)row_bytes);
    if (rows_per_item <= 0 || rows_per_item > rows) rows_per_item = rows;
    // strips as StftLaunch::launch cuts them: equal shares of at most 176 rows per strip, a whole number of strips per item
    const int target = 162;
    const int spi = (int)((rows_per_item + target - 1) / target);
    const int strip = (int)((rows_per_item + spi - 1) / spi);
    const long long items = (rows + rows_per_item - 1) / rows_per_item;
    const long long strips = items * spi, grid = (strips + 7) / 8 * 8;
    const int lds = (160 * 1024 / 12) & ~255;
    hipEvent_t e0, e1;
    LRA_HIP(hipEventCreate(&e0));
    LRA_HIP(hipEventCreate(&e1));
    float best = 0.f;
    for (int rep = 0; rep < 3; ++rep) {  // (the first repeat doubles as the warm-up: pages touched, clocks up)
        (void)hipEventRecord(e0, ctx->stream);
        for (int r = 0; r < 4; ++r) hipLaunchKernelGGL(placed_probe_kernel, dim3((unsigned)grid), dim3(64), lds, ctx->stream, (char*)ptr, rows, row_bytes, rows_per_item, strip, spi, (int)(grid / 8));
        (void)hipEventRecord(e1, ctx->stream);
        if (hipEventSynchronize(e1) != hipSuccess || hipGetLastError() != hipSuccess) {
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
            return fail(LRA_EHIP, "placement probe failed");
        }
        float t = 0.f;
        (void)hipEventElapsedTime(&t, e0, e1);
        if (rep == 1 || (rep > 1 && t / 4 < best)) best = t / 4;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms = best;
    return LRA_OK;
}
}  // namespace

int lra_malloc_placed(lra_ctx* ctx, size_t bytes, int row_bytes, int64_t rows_per_item, int tries, void** dptr, float* probe_ms, int* tried) {
    LRA_BIND(ctx);
    if (!dptr) return fail(LRA_EINVAL, "null dptr");
    *dptr = nullptr;
    if (ctx->opt_placement_retry > 0) tries = ctx->opt_placement_retry;
    if (tries < 1) tries = 1;
    if (tries > 8) tries = 8;
    if (row_bytes < 512 || (row_bytes & 7) || bytes < (size_t)row_bytes * 4096) return fail(LRA_EINVAL, "lra_malloc_placed: for buffers of at least 4096 rows of >= 512 bytes (a multiple of 8)");
    struct Cand { void* p; lra_ctx::PlacedAlloc pa; float ms; };
    std::vector<Cand> cands;
    int rc = LRA_OK, best = -1;
    // Candidates alternate between an ordinary hipMalloc block and a range assembled from 64 MiB physical handles.  Neither kind is better everywhere: on four boxes
    // the assembled ranges landed on the fastest level every time (0.624-0.639 ms for the complex STFT where hipMalloc blocks gave 0.616-0.734), on a fifth they sat on
    // its slowest (0.735 against 0.672-0.694 for hipMalloc, profiles/r06_raw/u_*): the write stream decides, per buffer.
    for (int i = 0; i < tries; ++i) {
        Cand c{nullptr, {}, 0.f};
        const bool plain = (i % 2) == 0;
        if (plain) {
            c.pa.plain = true;
            c.pa.padded = bytes;
            hipError_t e = hipMalloc(&c.p, bytes);
            rc = e == hipSuccess ? LRA_OK : fail(e == hipErrorOutOfMemory ? LRA_ENOMEM : LRA_EHIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        } else {
            rc = placed_create(ctx, bytes, (size_t)64 << 20, &c.p, &c.pa);
        }
        if (rc != LRA_OK) {
            if (!cands.empty()) { rc = LRA_OK; (void)hipGetLastError(); }  // (out of memory for one more candidate: keep the best so far)
            break;
        }
        rc = placed_probe_ms(ctx, c.p, bytes, row_bytes, (long long)rows_per_item, &c.ms);
        cands.push_back(c);
        if (rc != LRA_OK) break;
        if (best < 0 || c.ms < cands[best].ms) best = (int)cands.size() - 1;
        const double gbps = (double)bytes / (cands[best].ms * 1e-3) / 1e9;
        if (ctx->placed_best_gbps > 0 && gbps >= 0.985 * ctx->placed_best_gbps && cands.size() >= 2) break;  // as good as anything this context has seen
        if (cands.size() >= 2) {  // (one of each kind by now)
            float lo = cands[0].ms, hi = cands[0].ms;
            for (const Cand& k : cands) { lo = std::min(lo, k.ms); hi = std::max(hi, k.ms); }
            // candidates that agree = no placement lottery on this box -- unless this context has already seen a clearly faster buffer of this kind of stream
            if (hi <= 1.015f * lo && !(ctx->placed_best_gbps > 0 && gbps < 0.97 * ctx->placed_best_gbps)) break;
        }
    }
    if (rc != LRA_OK || best < 0) {
        for (Cand& c : cands) placed_release(ctx, c.p, c.pa);
        return rc != LRA_OK ? rc : fail(LRA_ENOMEM, "lra_malloc_placed: no candidate");
    }
    for (int i = 0; i < (int)cands.size(); ++i)
        if (i != best) placed_release(ctx, cands[i].p, cands[i].pa);
    ctx->placed_best_gbps = std::max(ctx->placed_best_gbps, (double)bytes / (cands[best].ms * 1e-3) / 1e9);
    {
        std::lock_guard<std::mutex> lk(ctx->placed_mu);
        ctx->placed[cands[best].p] = cands[best].pa;
    }
    *dptr = cands[best].p;
    if (probe_ms) *probe_ms = cands[best].ms;
    if (tried) *tried = (int)cands.size();
    return LRA_OK;
}

int lra_free_placed(lra_ctx* ctx, void* dptr) {
    LRA_BIND(ctx);
    if (!dptr) return LRA_OK;
    lra_ctx::PlacedAlloc pa;
    {
        std::lock_guard<std::mutex> lk(ctx->placed_mu);
        auto it = ctx->placed.find(dptr);
        if (it == ctx->placed.end()) return fail(LRA_EINVAL, "lra_free_placed: not a pointer from lra_malloc_placed of this context");
        pa = it->second;
        ctx->placed.erase(it);
    }
    LRA_HIP(hipDeviceSynchronize());  // (unmapping under running work faults; these are large, long-lived buffers)
    placed_release(ctx, dptr, pa);
    return LRA_OK;
}

int lra_memset(lra_ctx* ctx, void* dptr, int value, size_t bytes) {
    LRA_BIND(ctx);
    LRA_HIP(hipMemsetAsync(dptr, value, bytes, ctx->stream));
    return LRA_OK;
}

int lra_memcpy_h2d(lra_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes) {
    LRA_BIND(ctx);
    LRA_HIP(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    LRA_HIP(hipStreamSynchronize(ctx->stream));
    return LRA_OK;
}

int lra_memcpy_d2h(lra_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes) {
    LRA_BIND(ctx);
    LRA_HIP(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    LRA_HIP(hipStreamSynchronize(ctx->stream));
    return LRA_OK;
}

int lra_event_create(lra_ctx* ctx, lra_event** out) {
    LRA_BIND(ctx);
    if (!out) return fail(LRA_EINVAL, "null out");
    lra_event* e = new lra_event();
    e->ctx = ctx;
    hipError_t err = hipEventCreate(&e->ev);
    if (err != hipSuccess) {
        delete e;
        return fail(LRA_EHIP, std::string("hipEventCreate: ") + hipGetErrorString(err));
    }
    *out = e;
    return LRA_OK;
}

void lra_event_destroy(lra_event* ev) {
    if (!ev) return;
    (void)hipEventDestroy(ev->ev);
    delete ev;
}

int lra_event_record(lra_event* ev) {
    if (!ev) return fail(LRA_EINVAL, "null event");
    LRA_BIND(ev->ctx);
    LRA_HIP(hipEventRecord(ev->ev, ev->ctx->stream));
    return LRA_OK;
}

int lra_event_elapsed_ms(lra_event* start, lra_event* stop, float* ms) {
    if (!start || !stop || !ms) return fail(LRA_EINVAL, "null argument");
    LRA_BIND(stop->ctx);
    LRA_HIP(hipEventSynchronize(stop->ev));
    LRA_HIP(hipEventElapsedTime(ms, start->ev, stop->ev));
    return LRA_OK;
}

// ---- STFT ---------------------------------------------------------------------------------------
namespace {
// twiddle tables of the mixed-radix kernels on the device: mixed::fill_twiddles (lra_mixed.h), uploaded
int mixed_tables(int n_fft, int dtype, void** d_mtw, void** d_mtwn) {
    auto fill_and_upload = [&](auto real) -> int {
        using T = decltype(real);
        std::vector<mixed::cpx<T>> t1(n_fft / 2), t2(n_fft / 2 + 1);
        mixed::fill_twiddles<T>(n_fft, t1.data(), t2.data());
        LRA_TRY(upload(d_mtw, t1.data(), t1.size() * sizeof(mixed::cpx<T>)));
        return upload(d_mtwn, t2.data(), t2.size() * sizeof(mixed::cpx<T>));
    };
    return dtype == LRA_F64 ? fill_and_upload(double()) : fill_and_upload(float());
}
}  // namespace

extern "C++" {  // (lra_internal.h: shared with the feature units)
int lra::ctx_twiddles(lra_ctx* ctx, int n_fft, int dtype, const void** tw_m, const void** tw_n) {
    auto& tw = ctx->cqt_tw[std::make_pair(n_fft, dtype)];
    if (!tw.first) LRA_TRY(mixed_tables(n_fft, dtype, &tw.first, &tw.second));
    *tw_m = tw.first;
    *tw_n = tw.second;
    return LRA_OK;
}

int lra::read_status(lra_ctx* ctx, const void* dev, void* host, size_t bytes) {
    LRA_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    LRA_HIP(hipStreamSynchronize(ctx->stream));
    return LRA_OK;
}
}  // extern "C++"

int lra_stft_plan_create(lra_ctx* ctx, int n_fft, int hop_length, const void* window_host, int center, int pad_mode, int dtype, lra_stft_plan** out) {
    LRA_BIND(ctx);
    if (!out) return fail(LRA_EINVAL, "null out");
    *out = nullptr;
    if (n_fft < 1) return fail(LRA_EINVAL, "n_fft must be positive");
    if (hop_length < 1) return fail(LRA_EINVAL, "hop_length=" + std::to_string(hop_length) + " must be a positive integer");
    if (!window_host) return fail(LRA_EINVAL, "null window");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "bad dtype");
    if (pad_mode < LRA_PAD_CONSTANT || pad_mode > LRA_PAD_SYMMETRIC) return fail(LRA_EINVAL, "bad pad_mode");
    lra_stft_plan* p = new lra_stft_plan();
    p->ctx = ctx;
    p->n_fft = n_fft;
    p->hop = hop_length;
    p->center = center ? 1 : 0;
    p->pad_mode = pad_mode;
    p->dtype = dtype;
    p->pow2 = pow2_supported(n_fft, dtype == LRA_F64);
    int rc;
    if (p->pow2) {
        // the fused kernels take 0.5 * window: the 1/2 of the real-FFT split step, folded in (exact)
        if (dtype == LRA_F64) {
            std::vector<double> wh(n_fft);
            for (int i = 0; i < n_fft; ++i) wh[i] = 0.5 * ((const double*)window_host)[i];
            rc = upload(&p->d_win, wh.data(), wh.size() * sizeof(double));
        } else {
            std::vector<float> wh(n_fft);
            for (int i = 0; i < n_fft; ++i) wh[i] = 0.5f * ((const float*)window_host)[i];
            rc = upload(&p->d_win, wh.data(), wh.size() * sizeof(float));
        }
    } else {
        rc = upload(&p->d_win, window_host, (size_t)n_fft * real_bytes(dtype));
    }
    if (rc == LRA_OK && ((!p->pow2 && mixed::in_size_list(n_fft)) || (p->pow2 && mixed::in_fwd_pow2_list(n_fft)))) rc = mixed_tables(n_fft, dtype, &p->d_mtw, &p->d_mtwn);
    if (rc == LRA_OK && p->pow2 && mixed::in_fwd_pow2_list(n_fft)) rc = upload(&p->d_win_full, window_host, (size_t)n_fft * real_bytes(dtype));
    if (rc == LRA_OK && p->pow2) {
        p->logm = log2_exact(n_fft) - 1;
        rc = dtype == LRA_F64 ? build_tables<double>(p->logm, p->d_tw, &p->d_twr) : build_tables<float>(p->logm, p->d_tw, &p->d_twr);
    }
    if (rc != LRA_OK) {
        lra_stft_plan_destroy(p);
        return rc;
    }
    *out = p;
    return LRA_OK;
}

void lra_stft_plan_destroy(lra_stft_plan* p) {
    if (!p) return;
    DeviceGuard device_guard__(p->ctx->device);
    if (p->d_win) (void)hipFree(p->d_win);
    if (p->d_win_full) (void)hipFree(p->d_win_full);
    for (int v = 0; v < kNumVariants; ++v)
        if (p->d_tw[v]) (void)hipFree(p->d_tw[v]);
    if (p->d_twr) (void)hipFree(p->d_twr);
    if (p->d_mtw) (void)hipFree(p->d_mtw);
    if (p->d_mtwn) (void)hipFree(p->d_mtwn);
    delete p;
}

int lra_stft_num_frames(const lra_stft_plan* p, int64_t n, int64_t* n_frames) {
    if (!p || !n_frames) return fail(LRA_EINVAL, "null argument");
    if (n < 0) return fail(LRA_EINVAL, "negative signal length");
    const int64_t padded = n + (p->center ? 2 * (int64_t)(p->n_fft / 2) : 0);
    if (padded < p->n_fft) {
        if (p->center) return fail(LRA_EINVAL, "Input is too short (n=" + std::to_string(padded) + ") for frame_length=" + std::to_string(p->n_fft));
        return fail(LRA_EINVAL, "n_fft=" + std::to_string(p->n_fft) + " is too large for uncentered analysis of input signal of length=" + std::to_string(n));
    }
    *n_frames = 1 + (padded - p->n_fft) / p->hop;
    return LRA_OK;
}

int lra_stft_plan_is_fused(const lra_stft_plan* p) { return p && p->pow2 ? 1 : 0; }
int lra_stft_plan_tuned_variant(const lra_stft_plan* p, int mode) {
    if (!p || mode < 0 || mode > 2) return -1;
    // the two-slope mel kernel is mode 3 internally; the banded one mode 2
    if (mode == 2) return p->tuned_variant[3] >= 0 ? p->tuned_variant[3] : p->tuned_variant[2];
    return p->tuned_variant[mode];
}
int lra_istft_plan_tuned_variant(const lra_istft_plan* p) { return p ? p->tuned_variant[0] : -1; }

int lra_stft_exec(lra_stft_plan* p, const void* y, int64_t batch, int64_t n, int64_t y_stride, void* D) {
    if (!p) return fail(LRA_EINVAL, "null plan");
    return p->dtype == LRA_F64 ? stft_run<double>(p, OUT_COMPLEX, y, batch, n, y_stride, 1.0, nullptr, D)
                               : stft_run<float>(p, OUT_COMPLEX, y, batch, n, y_stride, 1.0, nullptr, D);
}

int lra_spectrogram_exec(lra_stft_plan* p, const void* y, int64_t batch, int64_t n, int64_t y_stride, double power, void* S) {
    if (!p) return fail(LRA_EINVAL, "null plan");
    return p->dtype == LRA_F64 ? stft_run<double>(p, OUT_POWER, y, batch, n, y_stride, power, nullptr, S)
                               : stft_run<float>(p, OUT_POWER, y, batch, n, y_stride, power, nullptr, S);
}

int lra_stft_exec_strided(lra_stft_plan* p, int kind, const void* y, int64_t batch, int64_t n, int64_t y_stride, double power, void* out, int64_t out_frame_stride) {
    if (!p) return fail(LRA_EINVAL, "null plan");
    if (kind != 0 && kind != 1) return fail(LRA_EINVAL, "kind must be 0 (complex) or 1 (|X|^power)");
    const int mode = kind == 0 ? OUT_COMPLEX : OUT_POWER;
    return p->dtype == LRA_F64 ? stft_run<double>(p, mode, y, batch, n, y_stride, kind ? power : 1.0, nullptr, out, out_frame_stride)
                               : stft_run<float>(p, mode, y, batch, n, y_stride, kind ? power : 1.0, nullptr, out, out_frame_stride);
}

// ---- mel ----------------------------------------------------------------------------------------
int lra_mel_plan_create(lra_ctx* ctx, int n_mels, int n_bins, const void* basis_host, int dtype, lra_mel_plan** out) {
    LRA_BIND(ctx);
    if (!out) return fail(LRA_EINVAL, "null out");
    *out = nullptr;
    if (n_mels < 1 || n_bins < 1 || !basis_host) return fail(LRA_EINVAL, "bad mel basis");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "bad dtype");
    std::vector<int> c0(n_mels, 0), len(n_mels, 0), off(n_mels, 0);
    std::vector<char> vals;
    const size_t es = real_bytes(dtype);
    const char* B = (const char*)basis_host;
    auto nonzero = [&](int m, int c) {
        return dtype == LRA_F64 ? ((const double*)B)[(size_t)m * n_bins + c] != 0.0 : ((const float*)B)[(size_t)m * n_bins + c] != 0.0f;
    };
    int pos = 0;
    for (int m = 0; m < n_mels; ++m) {
        int first = -1, last = -1;
        for (int c = 0; c < n_bins; ++c)
            if (nonzero(m, c)) {
                if (first < 0) first = c;
                last = c;
            }
        off[m] = pos;
        if (first >= 0) {
            c0[m] = first;
            len[m] = last - first + 1;
            vals.insert(vals.end(), B + ((size_t)m * n_bins + first) * es, B + ((size_t)m * n_bins + last + 1) * es);
            pos += len[m];
        }
    }
    lra_mel_plan* p = new lra_mel_plan();
    p->ctx = ctx;
    p->n_mels = n_mels;
    p->n_bins = n_bins;
    p->dtype = dtype;
    int rc = upload((void**)&p->d_c0, c0.data(), c0.size() * sizeof(int));
    if (rc == LRA_OK) rc = upload((void**)&p->d_len, len.data(), len.size() * sizeof(int));
    if (rc == LRA_OK) rc = upload((void**)&p->d_off, off.data(), off.size() * sizeof(int));
    if (rc == LRA_OK) rc = upload(&p->d_val, vals.data(), vals.size());
    p->nnz = (int)(vals.size() / (dtype == LRA_F64 ? 8 : 4));
    if (rc == LRA_OK) {
        if (dtype == LRA_F64) {
            TwoSlope<double> ts = build_two_slope<double>((const double*)basis_host, n_mels, n_bins);
            if (ts.ok) {
                rc = upload(&p->d_wAB, ts.wAB.data(), ts.wAB.size() * sizeof(double));
                for (int pi = 0; pi < 2 && rc == LRA_OK; ++pi) {
                    const int bpl = pi == 0 ? 8 : 16;
                    if ((n_bins - 1) % bpl) continue;
                    MelPieces mp = build_mel_pieces<double>(ts, (n_bins - 1) / bpl, bpl);
                    if (mp.n_pieces <= 0) continue;
                    rc = upload((void**)&p->d_run[pi], mp.run_desc.data(), mp.run_desc.size() * sizeof(int));
                    if (rc == LRA_OK) rc = upload((void**)&p->d_segd[pi], mp.seg_desc.data(), mp.seg_desc.size() * sizeof(int));
                    p->nyq[pi] = mp.nyquist_piece;
                    p->n_pieces[pi] = mp.n_pieces;
                }
                if (rc == LRA_OK && (n_bins - 1) % 16 == 0) {
                    MelRuns<double> mr = build_mel_runs<double>(ts, (n_bins - 1) / 16, 8, MELR_PMAX, melr_ph_of_tf((n_bins - 1) / 16));  // (min list length = the hoisted prefix)
                    if (mr.ok) {
                        rc = upload(&p->d_melr_w, mr.w.data(), mr.w.size() * sizeof(double));
                        if (rc == LRA_OK) rc = upload(&p->d_melr_keep, mr.keep.data(), mr.keep.size() * sizeof(double));
                        if (rc == LRA_OK) rc = upload((void**)&p->d_melr_addr, mr.addr.data(), mr.addr.size() * sizeof(int));
                        p->melr_zero = mr.zero_addr;
                        p->melr_mid = mr.mid_addr;
                        p->melr_pmax = mr.pmax;
                        p->melr_ok = rc == LRA_OK;
                    }
                    MelRuns<double> mr2 = build_mel_runs<double>(ts, (n_bins - 1) / 16, 8, MELR_PMAX, 4, 1);
                    if (rc == LRA_OK && mr2.ok) {
                        rc = upload(&p->d_melr2_w, mr2.w.data(), mr2.w.size() * sizeof(double));
                        if (rc == LRA_OK) rc = upload(&p->d_melr2_keep, mr2.keep.data(), mr2.keep.size() * sizeof(double));
                        if (rc == LRA_OK) rc = upload((void**)&p->d_melr2_addr, mr2.addr.data(), mr2.addr.size() * sizeof(int));
                        p->melr2_zero = mr2.zero_addr;
                        p->melr2_mid = mr2.mid_addr;
                        p->melr2_pmax = mr2.pmax;
                        p->melr2_ok = rc == LRA_OK;
                    }
                }
                p->two_slope = rc == LRA_OK;
            }
        } else {
            TwoSlope<float> ts = build_two_slope<float>((const float*)basis_host, n_mels, n_bins);
            if (ts.ok) {
                rc = upload(&p->d_wAB, ts.wAB.data(), ts.wAB.size() * sizeof(float));
                for (int pi = 0; pi < 2 && rc == LRA_OK; ++pi) {
                    const int bpl = pi == 0 ? 8 : 16;
                    if ((n_bins - 1) % bpl) continue;
                    MelPieces mp = build_mel_pieces<float>(ts, (n_bins - 1) / bpl, bpl);
                    if (mp.n_pieces <= 0) continue;
                    rc = upload((void**)&p->d_run[pi], mp.run_desc.data(), mp.run_desc.size() * sizeof(int));
                    if (rc == LRA_OK) rc = upload((void**)&p->d_segd[pi], mp.seg_desc.data(), mp.seg_desc.size() * sizeof(int));
                    p->nyq[pi] = mp.nyquist_piece;
                    p->n_pieces[pi] = mp.n_pieces;
                }
                if (rc == LRA_OK && (n_bins - 1) % 16 == 0) {
                    // n_fft = 512 with MANY bands: eight bands per thread (MelManyCfgOf).  Same box: 128 bands 1.54 -> 1.04 ms, but 80 bands 0.75 -> 1.18 (their wider pair segments need
                    // the longer hoisted lists of the four-band form; 97 bands 0.90 -> 1.02, 112 bands 1.23 -> 1.03): taken above 100 bands
                    p->melr_many = ctx->opt_mel_many && (n_bins - 1) / 16 == 16 && n_mels > 100;  // [sel:mel-many-plan]
                    MelRuns<float> mr = build_mel_runs<float>(ts, (n_bins - 1) / 16, 8, MELR_PMAX, melr_ph_of_tf((n_bins - 1) / 16, p->melr_many));  // (min list length = the hoisted prefix)
                    if (mr.ok) {
                        rc = upload(&p->d_melr_w, mr.w.data(), mr.w.size() * sizeof(float));
                        if (rc == LRA_OK) rc = upload(&p->d_melr_keep, mr.keep.data(), mr.keep.size() * sizeof(float));
                        if (rc == LRA_OK) rc = upload((void**)&p->d_melr_addr, mr.addr.data(), mr.addr.size() * sizeof(int));
                        p->melr_zero = mr.zero_addr;
                        p->melr_mid = mr.mid_addr;
                        p->melr_pmax = mr.pmax;
                        p->melr_ok = rc == LRA_OK;
                    }
                    MelRuns<float> mr2 = build_mel_runs<float>(ts, (n_bins - 1) / 16, 8, MELR_PMAX, 4, 1);
                    if (rc == LRA_OK && mr2.ok) {
                        rc = upload(&p->d_melr2_w, mr2.w.data(), mr2.w.size() * sizeof(float));
                        if (rc == LRA_OK) rc = upload(&p->d_melr2_keep, mr2.keep.data(), mr2.keep.size() * sizeof(float));
                        if (rc == LRA_OK) rc = upload((void**)&p->d_melr2_addr, mr2.addr.data(), mr2.addr.size() * sizeof(int));
                        p->melr2_zero = mr2.zero_addr;
                        p->melr2_mid = mr2.mid_addr;
                        p->melr2_pmax = mr2.pmax;
                        p->melr2_ok = rc == LRA_OK;
                    }
                }
                p->two_slope = rc == LRA_OK;
            }
        }
    }
    if (rc != LRA_OK) {
        lra_mel_plan_destroy(p);
        return rc;
    }
    *out = p;
    return LRA_OK;
}

void lra_mel_plan_destroy(lra_mel_plan* p) {
    if (!p) return;
    DeviceGuard device_guard__(p->ctx->device);
    if (p->d_c0) (void)hipFree(p->d_c0);
    if (p->d_len) (void)hipFree(p->d_len);
    if (p->d_off) (void)hipFree(p->d_off);
    if (p->d_val) (void)hipFree(p->d_val);
    if (p->d_wAB) (void)hipFree(p->d_wAB);
    if (p->d_melr_w) (void)hipFree(p->d_melr_w);
    if (p->d_melr_keep) (void)hipFree(p->d_melr_keep);
    if (p->d_melr_addr) (void)hipFree(p->d_melr_addr);
    if (p->d_melr2_w) (void)hipFree(p->d_melr2_w);
    if (p->d_melr2_keep) (void)hipFree(p->d_melr2_keep);
    if (p->d_melr2_addr) (void)hipFree(p->d_melr2_addr);
    for (int pi = 0; pi < 2; ++pi) {
        if (p->d_run[pi]) (void)hipFree(p->d_run[pi]);
        if (p->d_segd[pi]) (void)hipFree(p->d_segd[pi]);
    }
    delete p;
}

int lra_melspectrogram_exec(lra_stft_plan* stft, lra_mel_plan* mel, const void* y, int64_t batch, int64_t n, int64_t y_stride, double power, void* M) {
    if (!stft || !mel) return fail(LRA_EINVAL, "null plan");
    return stft->dtype == LRA_F64 ? stft_run<double>(stft, OUT_MEL, y, batch, n, y_stride, power, mel, M)
                                  : stft_run<float>(stft, OUT_MEL, y, batch, n, y_stride, power, mel, M);
}

int lra_stft_exec_host(lra_stft_plan* p, lra_mel_plan* mel, int kind, const void* y_host, int64_t batch, int64_t n, int64_t y_stride, double power, void* out_host,
                       int64_t out_item_stride, int* nonfinite) {
    if (!p) return fail(LRA_EINVAL, "null plan");
    lra_ctx* ctx = p->ctx;
    LRA_BIND(ctx);
    if (nonfinite) *nonfinite = 0;
    if (kind < 0 || kind > 2) return fail(LRA_EINVAL, "kind must be 0 (complex), 1 (|X|^power) or 2 (mel)");
    if (kind == 2 && !mel) return fail(LRA_EINVAL, "null mel plan");
    if (batch <= 0) return LRA_OK;
    if (!y_host || !out_host) return fail(LRA_EINVAL, "null data pointer");
    int64_t T = 0;
    LRA_TRY(lra_stft_num_frames(p, n, &T));
    const size_t es = real_bytes(p->dtype);
    const int64_t n_bins = p->n_fft / 2 + 1;
    const size_t in_item = (size_t)n * es;
    const size_t out_item = kind == 0 ? (size_t)T * n_bins * 2 * es : kind == 1 ? (size_t)T * n_bins * es : (size_t)T * mel->n_mels * es;
    if (out_item_stride <= 0) out_item_stride = (int64_t)(out_item / es);
    if ((size_t)out_item_stride * es < out_item) return fail(LRA_EINVAL, "out_item_stride smaller than one item");
    const int mode = kind == 0 ? OUT_COMPLEX : kind == 1 ? OUT_POWER : OUT_MEL;
    bool bad_samples = false;
    LRA_TRY(host_pipeline(ctx, batch, in_item, (size_t)y_stride * es, out_item, (size_t)out_item_stride * es, (const char*)y_host, (char*)out_host, nonfinite ? (int)es : 0, &bad_samples,
                          [&](void* d_in, void* d_out, int64_t, int64_t nb) -> int {
                              return p->dtype == LRA_F64 ? stft_run<double>(p, mode, d_in, nb, n, n, power, kind == 2 ? mel : nullptr, d_out)
                                                         : stft_run<float>(p, mode, d_in, nb, n, n, power, kind == 2 ? mel : nullptr, d_out);
                          }));
    if (nonfinite) *nonfinite = bad_samples ? 1 : 0;
    return LRA_OK;
}

int lra_mel_apply_exec(lra_mel_plan* mel, const void* S, int64_t batch, int64_t n_frames, int64_t batch_stride, int64_t bin_stride, int64_t frame_stride,
                       void* M) {
    if (!mel) return fail(LRA_EINVAL, "null plan");
    LRA_BIND(mel->ctx);
    if (batch <= 0 || n_frames <= 0) return LRA_OK;
    if (!S || !M) return fail(LRA_EINVAL, "null data pointer");
    const long long tblocks = (n_frames + 255) / 256;
    const long long grid = tblocks * mel->n_mels * batch;
    if (grid > 0x7fffffffLL) return fail(LRA_EINVAL, "grid too large");
    if (mel->dtype == LRA_F64)
        hipLaunchKernelGGL(mel_apply_kernel<double>, dim3((unsigned)grid), dim3(256), 0, mel->ctx->stream, (const double*)S, (long long)batch_stride,
                           (long long)bin_stride, (long long)frame_stride, (long long)n_frames, mel->n_mels, mel->d_c0, mel->d_len, mel->d_off,
                           (const double*)mel->d_val, (double*)M);
    else
        hipLaunchKernelGGL(mel_apply_kernel<float>, dim3((unsigned)grid), dim3(256), 0, mel->ctx->stream, (const float*)S, (long long)batch_stride,
                           (long long)bin_stride, (long long)frame_stride, (long long)n_frames, mel->n_mels, mel->d_c0, mel->d_len, mel->d_off,
                           (const float*)mel->d_val, (float*)M);
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

// ---- ISTFT --------------------------------------------------------------------------------------
int lra_istft_plan_create(lra_ctx* ctx, int n_fft, int hop_length, const void* window_host, int center, int dtype, lra_istft_plan** out) {
    LRA_BIND(ctx);
    if (!out) return fail(LRA_EINVAL, "null out");
    *out = nullptr;
    if (n_fft < 1) return fail(LRA_EINVAL, "n_fft must be positive");
    if (hop_length < 1) return fail(LRA_EINVAL, "hop_length must be a positive integer");
    if (!window_host) return fail(LRA_EINVAL, "null window");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "bad dtype");
    lra_istft_plan* p = new lra_istft_plan();
    p->ctx = ctx;
    p->n_fft = n_fft;
    p->hop = hop_length;
    p->center = center ? 1 : 0;
    p->dtype = dtype;
    p->pow2 = pow2_supported(n_fft, dtype == LRA_F64);
    int rc;
    if (dtype == LRA_F64) {
        std::vector<double> ws(n_fft);
        for (int i = 0; i < n_fft; ++i) ws[i] = ((const double*)window_host)[i] / (double)n_fft;
        rc = upload(&p->d_win_scaled, ws.data(), ws.size() * sizeof(double));
    } else {
        std::vector<float> ws(n_fft);
        for (int i = 0; i < n_fft; ++i) ws[i] = (float)((double)((const float*)window_host)[i] / (double)n_fft);
        rc = upload(&p->d_win_scaled, ws.data(), ws.size() * sizeof(float));
    }
    if (rc == LRA_OK && p->pow2) {
        p->logm = log2_exact(n_fft) - 1;
        rc = dtype == LRA_F64 ? build_tables<double>(p->logm, p->d_tw, &p->d_twr) : build_tables<float>(p->logm, p->d_tw, &p->d_twr);
    }
    if (rc == LRA_OK && ((!p->pow2 && mixed::in_size_list(n_fft)) || (p->pow2 && mixed::in_inv_pow2_list(n_fft)))) rc = mixed_tables(n_fft, dtype, &p->d_mtw, &p->d_mtwn);
    if (rc != LRA_OK) {
        lra_istft_plan_destroy(p);
        return rc;
    }
    *out = p;
    return LRA_OK;
}

void lra_istft_plan_destroy(lra_istft_plan* p) {
    if (!p) return;
    DeviceGuard device_guard__(p->ctx->device);
    if (p->d_win_scaled) (void)hipFree(p->d_win_scaled);
    for (int v = 0; v < kNumVariants; ++v)
        if (p->d_tw[v]) (void)hipFree(p->d_tw[v]);
    if (p->d_twr) (void)hipFree(p->d_twr);
    if (p->d_mtw) (void)hipFree(p->d_mtw);
    if (p->d_mtwn) (void)hipFree(p->d_mtwn);
    delete p;
}

int lra_istft_exec(lra_istft_plan* p, const void* D, int64_t batch, int64_t d_batch_stride, int64_t d_frame_stride, int64_t n_used, const void* wss,
                   void* y, int64_t out_len, int64_t y_stride) {
    if (!p) return fail(LRA_EINVAL, "null plan");
    return p->dtype == LRA_F64 ? istft_run<double>(p, D, batch, d_batch_stride, d_frame_stride, n_used, wss, 0, y, out_len, y_stride)
                               : istft_run<float>(p, D, batch, d_batch_stride, d_frame_stride, n_used, wss, 0, y, out_len, y_stride);
}

int lra_istft_exec_norm(lra_istft_plan* p, const void* D, int64_t batch, int64_t d_batch_stride, int64_t d_frame_stride, int64_t n_used, const void* norm,
                   void* y, int64_t out_len, int64_t y_stride) {
    if (!p) return fail(LRA_EINVAL, "null plan");
    return p->dtype == LRA_F64 ? istft_run<double>(p, D, batch, d_batch_stride, d_frame_stride, n_used, norm, 1, y, out_len, y_stride)
                               : istft_run<float>(p, D, batch, d_batch_stride, d_frame_stride, n_used, norm, 1, y, out_len, y_stride);
}

int lra_istft_exec_host(lra_istft_plan* p, const void* D_host, int64_t batch, int64_t n_frames, int64_t n_used, const void* wss_host, void* y_host, int64_t out_len,
                        int64_t y_stride) {
    if (!p) return fail(LRA_EINVAL, "null plan");
    lra_ctx* ctx = p->ctx;
    LRA_BIND(ctx);
    if (batch <= 0 || out_len <= 0) return LRA_OK;
    if (!D_host || !wss_host || !y_host) return fail(LRA_EINVAL, "null data pointer");
    if (n_frames <= 0 || n_used < 0 || n_used > n_frames) return fail(LRA_EINVAL, "bad frame counts");
    if (y_stride < out_len) return fail(LRA_EINVAL, "y_stride smaller than out_len");
    const size_t es = real_bytes(p->dtype);
    const int64_t n_bins = p->n_fft / 2 + 1;
    const size_t in_item = (size_t)n_frames * n_bins * 2 * es, out_item = (size_t)out_len * es;
    LRA_TRY(pipe_ensure(ctx, 16, 16));  // (creates the pipe; host_pipeline sizes the slots)
    HostPipe* hp = ctx->pipe;
    if (out_item > hp->aux_cap) {
        if (hp->dev_aux) (void)hipFree(hp->dev_aux);
        hp->dev_aux = nullptr;
        hp->aux_cap = 0;
        LRA_HIP(hipMalloc(&hp->dev_aux, out_item));
        hp->aux_cap = out_item;
    }
    LRA_HIP(hipMemcpyAsync(hp->dev_aux, wss_host, out_item, hipMemcpyHostToDevice, ctx->stream));
    return host_pipeline(ctx, batch, in_item, in_item, out_item, (size_t)y_stride * es, (const char*)D_host, (char*)y_host, 0, nullptr,
                         [&](void* d_in, void* d_out, int64_t, int64_t nb) -> int {
                             return p->dtype == LRA_F64 ? istft_run<double>(p, d_in, nb, n_frames * n_bins, n_bins, n_used, hp->dev_aux, 0, d_out, out_len, out_len)
                                                        : istft_run<float>(p, d_in, nb, n_frames * n_bins, n_bins, n_used, hp->dev_aux, 0, d_out, out_len, out_len);
                         });
}

// ---- decibel scaling and MFCC (lra_post.h) -------------------------------------------------------------------------
int lra_item_absmax_exec(lra_ctx* ctx, const void* x, int64_t batch, int64_t per_item, int dtype, void* out_max) { return lra_item_max_exec(ctx, x, batch, per_item, dtype, 1, out_max); }

int lra_item_max_exec(lra_ctx* ctx, const void* x, int64_t batch, int64_t per_item, int dtype, int absolute, void* out_max) {
    LRA_BIND(ctx);
    if (batch <= 0) return LRA_OK;
    if (!x || !out_max) return fail(LRA_EINVAL, "null data pointer");
    if (per_item <= 0) return fail(LRA_EINVAL, "empty items have no maximum");
    const int chunks = post_chunks(batch, per_item, ctx->n_cu);
    if (batch * chunks > 0x7fffffffLL) return fail(LRA_EINVAL, "too many items");
    LRA_HIP(hipMemsetAsync(out_max, 0, (size_t)batch * real_bytes(dtype), ctx->stream));
    const dim3 grid((unsigned)(batch * chunks)), block(256);
    if (dtype == LRA_F64) {
        if (absolute) hipLaunchKernelGGL((item_absmax_kernel<double, true>), grid, block, 0, ctx->stream, (const double*)x, (long long)per_item, chunks, (unsigned long long*)out_max);
        else hipLaunchKernelGGL((item_absmax_kernel<double, false>), grid, block, 0, ctx->stream, (const double*)x, (long long)per_item, chunks, (unsigned long long*)out_max);
    } else {
        if (absolute) hipLaunchKernelGGL((item_absmax_kernel<float, true>), grid, block, 0, ctx->stream, (const float*)x, (long long)per_item, chunks, (unsigned int*)out_max);
        else hipLaunchKernelGGL((item_absmax_kernel<float, false>), grid, block, 0, ctx->stream, (const float*)x, (long long)per_item, chunks, (unsigned int*)out_max);
    }
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

int lra_to_db_exec(lra_ctx* ctx, const void* x, void* out, int64_t batch, int64_t per_item, int dtype, int amplitude, double amin, double ref_scalar, const void* ref_items,
                   const void* item_max, int use_top_db, double top_db) {
    LRA_BIND(ctx);
    if (batch <= 0 || per_item <= 0) return LRA_OK;
    if (!x || !out) return fail(LRA_EINVAL, "null data pointer");
    if (!(amin > 0)) return fail(LRA_EINVAL, "amin must be strictly positive");
    if (use_top_db && top_db < 0) return fail(LRA_EINVAL, "top_db must be non-negative");
    if (use_top_db && !item_max) return fail(LRA_EINVAL, "top_db needs the per-item maxima");
    return dtype == LRA_F64 ? to_db_run<double>(ctx, x, out, batch, per_item, amplitude, amin, ref_scalar, ref_items, item_max, use_top_db, top_db)
                            : to_db_run<float>(ctx, x, out, batch, per_item, amplitude, amin, ref_scalar, ref_items, item_max, use_top_db, top_db);
}

int lra_from_db_exec(lra_ctx* ctx, const void* x, void* out, int64_t count, int dtype, int amplitude, double ref) {
    LRA_BIND(ctx);
    if (count <= 0) return LRA_OK;
    if (!x || !out) return fail(LRA_EINVAL, "null data pointer");
    long long grid = (count + 255) / 256;
    if (grid > 64LL * ctx->n_cu) grid = 64LL * ctx->n_cu;
#define LRA_FROM(T, AMP) hipLaunchKernelGGL((from_db_kernel<T, AMP>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, (const T*)x, (T*)out, (long long)count, (T)ref)
    if (dtype == LRA_F64) { if (amplitude) LRA_FROM(double, true); else LRA_FROM(double, false); }
    else { if (amplitude) LRA_FROM(float, true); else LRA_FROM(float, false); }
#undef LRA_FROM
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

int lra_griffinlim_update(lra_ctx* ctx, const void* rebuilt, const void* tprev, const void* S, void* angles, int64_t count, int dtype, double coef, double eps, int normalize) {
    LRA_BIND(ctx);
    if (count <= 0) return LRA_OK;
    if (!rebuilt || !S || !angles) return fail(LRA_EINVAL, "null data pointer");
    long long grid = (count + 255) / 256;
    if (grid > 64LL * ctx->n_cu) grid = 64LL * ctx->n_cu;
#define LRA_GL(T, N) hipLaunchKernelGGL((griffinlim_update_kernel<T, N>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, (const Cplx2<T>*)rebuilt, (const Cplx2<T>*)tprev, (const T*)S, (Cplx2<T>*)angles, (long long)count, (T)coef, (T)eps)
    if (dtype == LRA_F64) { if (normalize) LRA_GL(double, true); else LRA_GL(double, false); }
    else { if (normalize) LRA_GL(float, true); else LRA_GL(float, false); }
#undef LRA_GL
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

int lra_griffinlim_init(lra_ctx* ctx, const void* u, const void* S, void* angles, int64_t count, int dtype) {
    LRA_BIND(ctx);
    if (count <= 0) return LRA_OK;
    if (!u || !S || !angles) return fail(LRA_EINVAL, "null data pointer");
    long long grid = (count + 255) / 256;
    if (grid > 64LL * ctx->n_cu) grid = 64LL * ctx->n_cu;
    if (dtype == LRA_F64) hipLaunchKernelGGL((griffinlim_init_kernel<double>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, (const double*)u, (const double*)S, (Cplx2<double>*)angles, (long long)count);
    else hipLaunchKernelGGL((griffinlim_init_kernel<float>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, (const double*)u, (const float*)S, (Cplx2<float>*)angles, (long long)count);
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

int lra_pcg64_random_exec(lra_ctx* ctx, const uint64_t* state4, uint64_t offset, void* out, int64_t count) {
    LRA_BIND(ctx);
    if (count <= 0) return LRA_OK;
    if (!state4 || !out) return fail(LRA_EINVAL, "null argument");
    const rng::Pcg64 g{state4[0], state4[1], state4[2], state4[3]};
    const long long runs = (count + rng::kRunLength - 1) / rng::kRunLength;
    const long long grid = (runs + 255) / 256;
    if (grid > 0x7ffffff0LL) return fail(LRA_EINVAL, "too many draws for one call");
    hipLaunchKernelGGL(rng::pcg64_uniform_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, g, offset, (double*)out, (long long)count);
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

int lra_griffinlim_init_pcg64(lra_ctx* ctx, const uint64_t* state4, const void* S, void* angles, int64_t batch, int n_bins, int64_t n_frames, int dtype) {
    LRA_BIND(ctx);
    if (batch <= 0 || n_bins <= 0 || n_frames <= 0) return LRA_OK;
    if (!state4 || !S || !angles) return fail(LRA_EINVAL, "null argument");
    const rng::Pcg64 g{state4[0], state4[1], state4[2], state4[3]};
    // a thread owns `seg` consecutive frames of one (clip, bin) row: long enough that the jump-ahead (~2 x 27 128-bit products) is a small part of it,
    // short enough that the grid fills the chip (>= ~8 workgroups per CU where the job is that large)
    const int bin_blocks = (n_bins + 255) / 256;
    int seg = 256;
    while (seg > 32 && batch * bin_blocks * ((n_frames + seg - 1) / seg) < 8LL * ctx->n_cu) seg /= 2;
    const long long grid = batch * bin_blocks * ((n_frames + seg - 1) / seg);
    if (grid > 0x7ffffff0LL) return fail(LRA_EINVAL, "griffinlim init: grid too large");
    if (dtype == LRA_F64)
        hipLaunchKernelGGL((rng::griffinlim_init_pcg64_kernel<double>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, g, (const double*)S, (rng::RngCplx<double>*)angles, (long long)batch, n_bins,
                           (long long)n_frames, seg, bin_blocks);
    else
        hipLaunchKernelGGL((rng::griffinlim_init_pcg64_kernel<float>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, g, (const float*)S, (rng::RngCplx<float>*)angles, (long long)batch, n_bins,
                           (long long)n_frames, seg, bin_blocks);
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

int lra_phase_vocoder_exec(lra_ctx* ctx, const void* D, void* out, int64_t batch, int64_t n_frames, int n_bins, const double* t_out_host, int64_t n_out, int dtype) {
    LRA_BIND(ctx);
    if (batch <= 0 || n_out <= 0 || n_bins <= 0) return LRA_OK;
    if (!D || !out || !t_out_host) return fail(LRA_EINVAL, "null data pointer");
    if (n_frames < 2) return fail(LRA_EINVAL, "phase_vocoder needs at least two frames");
    // per output frame: the two phase frames and scipy interp1d's bracket (searchsorted left, clipped to [1, n - 1]; interpolate.py _call_linear)
    std::vector<VocoderStep<float>> steps((size_t)n_out);
    for (int64_t t = 0; t < n_out; ++t) {
        const double x = t_out_host[t];
        if (!(x >= 0) || !(x < (double)n_frames)) return fail(LRA_EINVAL, "t_out values must be in the range [0, D.shape[-1])");
        const int64_t i0 = (int64_t)std::floor(x);
        int64_t idx = (int64_t)std::ceil(x);  // first frame index >= x
        idx = std::min<int64_t>(std::max<int64_t>(idx, 1), n_frames - 1);
        steps[(size_t)t] = {(int)i0, (int)std::min<int64_t>(i0 + 1, n_frames - 1), (int)(idx - 1), x - (double)(idx - 1)};
    }
    void* d_steps = nullptr;
    LRA_HIP(hipMallocAsync(&d_steps, steps.size() * sizeof(steps[0]), ctx->stream));
    hipError_t e = hipMemcpyAsync(d_steps, steps.data(), steps.size() * sizeof(steps[0]), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // `steps` is pageable host memory that dies with this call
    if (e == hipSuccess) {
        const long long threads = (long long)batch * n_bins;
        const unsigned grid = (unsigned)((threads + 255) / 256);
        if (dtype == LRA_F64)
            hipLaunchKernelGGL(phase_vocoder_kernel<double>, dim3(grid), dim3(256), 0, ctx->stream, (const Cplx2<double>*)D, (Cplx2<double>*)out, (const VocoderStep<double>*)d_steps,
                               (long long)n_frames, (long long)n_out, n_bins, (long long)batch);
        else
            hipLaunchKernelGGL(phase_vocoder_kernel<float>, dim3(grid), dim3(256), 0, ctx->stream, (const Cplx2<float>*)D, (Cplx2<float>*)out, (const VocoderStep<float>*)d_steps,
                               (long long)n_frames, (long long)n_out, n_bins, (long long)batch);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(d_steps, ctx->stream);
    if (e != hipSuccess) return fail(LRA_EHIP, std::string("phase_vocoder: ") + hipGetErrorString(e));
    return LRA_OK;
}

int lra_pcen_exec(lra_ctx* ctx, const void* S, const void* ref, void* out, int64_t rows, int64_t n_frames, int dtype, double b, double gain, double bias, double power, double eps,
                  const void* zi, double zi_scalar, void* zf) {
    LRA_BIND(ctx);
    // the reference's own argument checks (:2598-2625); the shim raises ParameterError before getting here
    if (power < 0 || gain < 0 || bias < 0 || !(eps > 0) || !(b >= 0 && b <= 1)) return fail(LRA_EINVAL, "pcen: power, gain, bias must be non-negative, eps positive, b in [0, 1]");
    if (rows <= 0) return LRA_OK;
    if (n_frames <= 0) {  // no frames: the state passes through (scipy.signal.lfilter on an empty axis)
        if (zf) {
            if (zi) {
                LRA_HIP(hipMemcpyAsync(zf, zi, (size_t)rows * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
            } else {
                std::vector<double> fill((size_t)rows, zi_scalar);
                LRA_HIP(hipMemcpyAsync(zf, fill.data(), fill.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
                LRA_HIP(hipStreamSynchronize(ctx->stream));
            }
        }
        return LRA_OK;
    }
    if (!S || !out) return fail(LRA_EINVAL, "null data pointer");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "pcen: dtype must be LRA_F32 or LRA_F64");
    PcenArgs p;
    p.b = b;
    p.a1 = b - 1.0;
    p.zi_scalar = zi_scalar;
    p.neg_gain = -gain;
    p.log_eps = std::log(eps);
    p.eps = eps;
    p.power = power;
    p.bias = bias;
    p.bias_pow = std::pow(bias, power);
    p.mode = power == 0 ? 0 : (bias == 0 ? 1 : 2);
    const unsigned grid = (unsigned)((rows + kPcenRows - 1) / kPcenRows);
    if (dtype == LRA_F64)
        hipLaunchKernelGGL(pcen_kernel<double>, dim3(grid), dim3(64), 0, ctx->stream, (const double*)S, (const double*)(ref ? ref : S), (double*)out, (long long)rows, (long long)n_frames, p,
                           (const double*)zi, (double*)zf);
    else
        hipLaunchKernelGGL(pcen_kernel<float>, dim3(grid), dim3(64), 0, ctx->stream, (const float*)S, (const float*)(ref ? ref : S), (double*)out, (long long)rows, (long long)n_frames, p,
                           (const double*)zi, (double*)zf);
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

int lra_maxfilter_exec(lra_ctx* ctx, const void* S, void* out, int64_t outer, int n_bands, int64_t inner, int size, int dtype) {
    LRA_BIND(ctx);
    if (size < 1) return fail(LRA_EINVAL, "maxfilter: size must be a positive integer");
    if (outer <= 0 || n_bands <= 0 || inner <= 0) return LRA_OK;
    if (!S || !out) return fail(LRA_EINVAL, "null data pointer");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "maxfilter: dtype must be LRA_F32 or LRA_F64");
    const long long count = (long long)outer * n_bands * inner;
    if ((count + 255) / 256 > 0x7fffffffLL) return fail(LRA_EINVAL, "maxfilter: array too large for one launch");
    const unsigned grid = (unsigned)((count + 255) / 256);
    if (dtype == LRA_F64)
        hipLaunchKernelGGL(maxfilter_bands_kernel<double>, dim3(grid), dim3(256), 0, ctx->stream, (const double*)S, (double*)out, (long long)outer, n_bands, (long long)inner, size);
    else
        hipLaunchKernelGGL(maxfilter_bands_kernel<float>, dim3(grid), dim3(256), 0, ctx->stream, (const float*)S, (float*)out, (long long)outer, n_bands, (long long)inner, size);
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

// ---- onset strength (lra_onset.h) -------------------------------------------------------------------------------------------
static_assert(kOnsetNone == LRA_ONSET_NONE && kOnsetMean == LRA_ONSET_MEAN && kOnsetSum == LRA_ONSET_SUM && kOnsetMax == LRA_ONSET_MAX && kOnsetMin == LRA_ONSET_MIN &&
                  kOnsetMedian == LRA_ONSET_MEDIAN && kOnsetRows == LRA_ONSET_ROWS,
              "onset aggregation codes");
extern "C++" {  // (the launch templates; this part of the file is the C ABI)
namespace {
template <class T, bool DB>
int onset_run(lra_ctx* ctx, OnsetArgs<T> a, int aggregate, int max_ch_bands, int detrend, void* env, void* out) {
    const int rows = (aggregate == kOnsetNone || aggregate == kOnsetRows) ? a.n_bands : a.n_ch;
    a.out = detrend ? (T*)env : (T*)out;
    if (aggregate == kOnsetMedian) {
        const int fb = onset_median_frames(max_ch_bands, sizeof(T));
        const long long grid = a.batch * ((a.n_out + fb - 1) / fb);
        if (grid > 0x7fffffffLL) return fail(LRA_EINVAL, "onset: too many frames for one launch");
        const size_t lds = (size_t)(max_ch_bands > 0 ? max_ch_bands : 1) * fb * sizeof(T);
        const void* kern = reinterpret_cast<const void*>(&onset_median_kernel<T, DB>);
        if (lds > 65536) LRA_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((onset_median_kernel<T, DB>), dim3((unsigned)grid), dim3(fb), lds, ctx->stream, a);
    } else {
        const long long grid = a.batch * ((a.n_out + 255) / 256);
        if (grid > 0x7fffffffLL) return fail(LRA_EINVAL, "onset: too many frames for one launch");
#define LRA_ONSET(AGG) hipLaunchKernelGGL((onset_flux_kernel<T, DB, AGG>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, a)
        switch (aggregate) {
            case kOnsetNone: LRA_ONSET(kOnsetNone); break;
            case kOnsetMean: LRA_ONSET(kOnsetMean); break;
            case kOnsetSum: LRA_ONSET(kOnsetSum); break;
            case kOnsetMax: LRA_ONSET(kOnsetMax); break;
            case kOnsetMin: LRA_ONSET(kOnsetMin); break;
            default: LRA_ONSET(kOnsetRows); break;
        }
#undef LRA_ONSET
    }
    LRA_HIP(hipGetLastError());
    if (detrend) {
        const long long n_rows = a.batch * rows;
        const long long grid = (n_rows + kOnsetDetrendRows - 1) / kOnsetDetrendRows;
        if (grid > 0x7fffffffLL) return fail(LRA_EINVAL, "onset: too many rows for one launch");
        hipLaunchKernelGGL(onset_detrend_kernel<T>, dim3((unsigned)grid), dim3(64), 0, ctx->stream, (const T*)env, (double*)out, n_rows, (long long)a.n_out);
        LRA_HIP(hipGetLastError());
    }
    return LRA_OK;
}

template <class T>
int onset_dispatch(lra_ctx* ctx, const void* S, const void* ref, void* out, int64_t batch, int n_bands, int64_t n_frames, int lag, int max_size, int aggregate, const int32_t* ch_offsets,
                   const int32_t* ch_bands, int n_ch, int max_ch_bands, int64_t pad, int64_t n_out, int fuse_db, double amin, double top_db, const void* item_max, int detrend, void* env) {
    OnsetArgs<T> a;
    a.S = (const T*)S;
    a.ref = (const T*)ref;
    a.out = nullptr;
    a.ch_off = ch_offsets;
    a.ch_band = ch_bands;
    a.batch = batch;
    a.n_frames = n_frames;
    a.pad = pad;
    a.n_out = n_out;
    a.n_bands = n_bands;
    a.lag = aggregate == kOnsetRows ? 0 : lag;
    a.max_size = max_size;
    a.n_ch = n_ch;
    a.db = DbArgs<T>{(T)amin, (T)1, nullptr, (const T*)item_max, (T)top_db};
    return fuse_db ? onset_run<T, true>(ctx, a, aggregate, max_ch_bands, detrend, env, out) : onset_run<T, false>(ctx, a, aggregate, max_ch_bands, detrend, env, out);
}
}  // namespace
}  // extern "C++"

int lra_onset_exec(lra_ctx* ctx, const void* S, const void* ref, void* out, int64_t batch, int n_bands, int64_t n_frames, int dtype, int lag, int max_size, int aggregate,
                   const int32_t* ch_offsets, const int32_t* ch_bands, int n_ch, int max_ch_bands, int64_t pad, int64_t n_out, int fuse_db, double amin, double top_db,
                   const void* item_max, int detrend, void* env) {
    LRA_BIND(ctx);
    if (aggregate < LRA_ONSET_NONE || aggregate > LRA_ONSET_ROWS) return fail(LRA_EINVAL, "onset: unknown aggregate code");
    if (aggregate != LRA_ONSET_ROWS && (lag < 1 || max_size < 1)) return fail(LRA_EINVAL, "onset: lag and max_size must be positive integers");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "onset: dtype must be LRA_F32 or LRA_F64");
    if (n_bands < 0 || n_frames < 0 || pad < 0 || n_ch < 0) return fail(LRA_EINVAL, "onset: negative size");
    const bool per_band = aggregate == LRA_ONSET_NONE || aggregate == LRA_ONSET_ROWS;
    if (batch <= 0 || n_out <= 0 || (per_band ? n_bands : n_ch) == 0) return LRA_OK;
    if (!S || !out) return fail(LRA_EINVAL, "null data pointer");
    if (n_bands == 0) return fail(LRA_EINVAL, "onset: channels over an empty band axis");
    if (!per_band && (!ch_offsets != !ch_bands || max_ch_bands < 0)) return fail(LRA_EINVAL, "onset: give both channel tables or neither");
    if (!per_band && !ch_offsets && (n_ch != 1 || max_ch_bands != n_bands)) return fail(LRA_EINVAL, "onset: without channel tables there is one channel of every band");
    if (fuse_db && (!(amin > 0) || top_db < 0 || !item_max)) return fail(LRA_EINVAL, "onset: the decibel step needs amin > 0, top_db >= 0 and the per-item maxima");
    if (aggregate == LRA_ONSET_ROWS && fuse_db) return fail(LRA_EINVAL, "onset: finished rows take no decibel step");
    if (detrend && !env) return fail(LRA_EINVAL, "onset: detrend needs the envelope scratch");
    if (aggregate == LRA_ONSET_MEDIAN && onset_median_frames(max_ch_bands, real_bytes(dtype)) == 0)
        return fail(LRA_EINVAL, "onset: a median channel of " + std::to_string(max_ch_bands) + " bands does not fit the 160 KiB LDS of a CU");
    return dtype == LRA_F64 ? onset_dispatch<double>(ctx, S, ref, out, batch, n_bands, n_frames, lag, max_size, aggregate, ch_offsets, ch_bands, n_ch, max_ch_bands, pad, n_out, fuse_db,
                                                     amin, top_db, item_max, detrend, env)
                            : onset_dispatch<float>(ctx, S, ref, out, batch, n_bands, n_frames, lag, max_size, aggregate, ch_offsets, ch_bands, n_ch, max_ch_bands, pad, n_out, fuse_db,
                                                    amin, top_db, item_max, detrend, env);
}

int lra_fir_decimate_exec(lra_ctx* ctx, const void* x, void* out, int64_t batch, int64_t n_in, int64_t n_out, const void* taps, int n_taps, int down, int first, double div, double mul,
                          int dtype) {
    LRA_BIND(ctx);
    if (n_taps < 1 || down < 1 || first < 0 || !(div > 0)) return fail(LRA_EINVAL, "fir_decimate: n_taps and down must be positive, first non-negative, div positive");
    if (batch <= 0 || n_out <= 0) return LRA_OK;
    if (n_in <= 0) return fail(LRA_EINVAL, "fir_decimate: empty input");
    if (!x || !out || !taps) return fail(LRA_EINVAL, "null data pointer");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "fir_decimate: dtype must be LRA_F32 or LRA_F64");
    const FirPlan plan = fir_plan(n_out, n_taps, down, dtype == LRA_F64 ? 8 : 4);  // the kernel and its geometry (lra_cqt.h)
    const bool four = plan.opt == 4;
    const long long blocks_per_clip = plan.blocks_per_clip;
    const size_t lds = plan.lds_bytes;
    if (blocks_per_clip * batch > 0x7fffffffLL) return fail(LRA_EINVAL, "fir_decimate: array too large for one launch");
    const unsigned grid = (unsigned)(blocks_per_clip * batch);
    if (plan.route == kFirHalve4) {  // the octave recursion's halving: four consecutive outputs per thread, padded span of pairs
        if (dtype == LRA_F64)
            hipLaunchKernelGGL(fir_halve4_kernel<double>, dim3(grid), dim3(256), lds, ctx->stream, (const double*)x, (double*)out, (const double*)taps, (long long)n_in, (long long)n_out,
                               (int)blocks_per_clip, n_taps, first, div, mul);
        else
            hipLaunchKernelGGL(fir_halve4_kernel<float>, dim3(grid), dim3(256), lds, ctx->stream, (const float*)x, (float*)out, (const float*)taps, (long long)n_in, (long long)n_out,
                               (int)blocks_per_clip, n_taps, first, div, mul);
        LRA_HIP(hipGetLastError());
        return LRA_OK;
    }
    if (plan.route == kFirDirect) {  // span too long to stage
        const long long count = (long long)batch * n_out;
        if ((count + 255) / 256 > 0x7fffffffLL) return fail(LRA_EINVAL, "fir_decimate: array too large for one launch");
        const unsigned dgrid = (unsigned)((count + 255) / 256);
        if (dtype == LRA_F64)
            hipLaunchKernelGGL(fir_decimate_direct_kernel<double>, dim3(dgrid), dim3(256), 0, ctx->stream, (const double*)x, (double*)out, (const double*)taps, (long long)batch, (long long)n_in,
                               (long long)n_out, n_taps, down, first, div, mul);
        else
            hipLaunchKernelGGL(fir_decimate_direct_kernel<float>, dim3(dgrid), dim3(256), 0, ctx->stream, (const float*)x, (float*)out, (const float*)taps, (long long)batch, (long long)n_in,
                               (long long)n_out, n_taps, down, first, div, mul);
        LRA_HIP(hipGetLastError());
        return LRA_OK;
    }
#define LRA_FIR(T, OPT)                                                                                                                                                           \
    hipLaunchKernelGGL((fir_decimate_kernel<T, OPT>), dim3(grid), dim3(256), lds, ctx->stream, (const T*)x, (T*)out, (const T*)taps, (long long)n_in, (long long)n_out, (int)blocks_per_clip, \
                       n_taps, down, first, div, mul)
    if (dtype == LRA_F64) { if (four) LRA_FIR(double, 4); else LRA_FIR(double, 1); }
    else { if (four) LRA_FIR(float, 4); else LRA_FIR(float, 1); }
#undef LRA_FIR
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

int lra_resample_poly_exec(lra_ctx* ctx, const void* x, void* out, int64_t batch, int64_t n_in, int64_t n_out, const void* taps, int n_taps, int up, int down, int first, double div, double mul,
                           int dtype) {
    if (up == 1) return lra_fir_decimate_exec(ctx, x, out, batch, n_in, n_out, taps, n_taps, down, first, div, mul, dtype);  // the staged decimators
    LRA_BIND(ctx);
    if (n_taps < 1 || up < 1 || down < 1 || first < 0 || !(div > 0)) return fail(LRA_EINVAL, "resample_poly: n_taps, up and down must be positive, first non-negative, div positive");
    if (batch <= 0 || n_out <= 0) return LRA_OK;
    if (n_in <= 0) return fail(LRA_EINVAL, "resample_poly: empty input");
    if (!x || !out || !taps) return fail(LRA_EINVAL, "null data pointer");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "resample_poly: dtype must be LRA_F32 or LRA_F64");
    const long long count = (long long)batch * n_out;
    if ((count + 255) / 256 > 0x7fffffffLL) return fail(LRA_EINVAL, "resample_poly: array too large for one launch");
    const unsigned grid = (unsigned)((count + 255) / 256);
    if (dtype == LRA_F64)
        hipLaunchKernelGGL(resample_poly_kernel<double>, dim3(grid), dim3(256), 0, ctx->stream, (const double*)x, (double*)out, (const double*)taps, (long long)batch, (long long)n_in,
                           (long long)n_out, n_taps, up, down, first, div, mul);
    else
        hipLaunchKernelGGL(resample_poly_kernel<float>, dim3(grid), dim3(256), 0, ctx->stream, (const float*)x, (float*)out, (const float*)taps, (long long)batch, (long long)n_in,
                           (long long)n_out, n_taps, up, down, first, div, mul);
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

}  // extern "C"

namespace {
// the band-limited form (resample_shaped_spectrum_kernel): clips padded to fft_in, shaped, inverted at fft_out, the first n_out samples kept
template <class T>
int resample_shaped_run(lra_ctx* ctx, const T* x, T* out, long long batch, long long n_in, long long n_out, long long fft_in, long long fft_out, double k_mid, double k_sigma, double gain, int dtype) {
    if (!ctx->rs_fft) ctx->rs_fft = new ResampleFft();
    ResampleFft* rs = ctx->rs_fft;
    const long long bins_in = fft_in / 2 + 1, bins_out = fft_out / 2 + 1;
    long long per_pass = (1LL << 30) / ((bins_in + bins_out) * (long long)sizeof(cx<T>) + (fft_in + fft_out) * (long long)sizeof(T));
    if (per_pass < 1) per_pass = 1;
    if (per_pass > batch) per_pass = batch;
    LRA_TRY(scratch_acquire(rs->order, ctx->stream));
    LRA_TRY(rs->spec_in.ensure((size_t)per_pass * bins_in * sizeof(cx<T>)));
    LRA_TRY(rs->spec_out.ensure((size_t)per_pass * bins_out * sizeof(cx<T>)));
    LRA_TRY(rs->time_in.ensure((size_t)per_pass * fft_in * sizeof(T)));
    LRA_TRY(rs->time_out.ensure((size_t)per_pass * fft_out * sizeof(T)));
    const long long n_copy = (fft_out < fft_in ? fft_out : fft_in) / 2 + 1;
    const long long real_last = fft_out % 2 == 0 ? fft_out / 2 : -1;
    FftPlanCache* fwd = rs->get((int)rocfft_transform_type_real_forward, dtype, fft_in);
    FftPlanCache* inv = rs->get((int)rocfft_transform_type_real_inverse, dtype, fft_out);
    auto blocks = [](long long count) { return dim3((unsigned)((count + 255) / 256)); };
    for (long long c0 = 0; c0 < batch; c0 += per_pass) {
        const long long cnt = batch - c0 < per_pass ? batch - c0 : per_pass;
        hipLaunchKernelGGL(repitch_rows_kernel<T>, blocks(cnt * fft_in), dim3(256), 0, ctx->stream, x + c0 * n_in, (T*)rs->time_in.p, cnt, n_in, n_in, fft_in);
        rocfft_plan plan;
        LRA_TRY(get_rocfft_plan(*fwd, ctx, rocfft_transform_type_real_forward, dtype, (int)fft_in, cnt, &plan));
        void* ib[1] = {rs->time_in.p};
        void* ob[1] = {rs->spec_in.p};
        LRA_FFT(rocfft_execute(plan, ib, ob, fwd->info));
        hipLaunchKernelGGL(resample_shaped_spectrum_kernel<T>, blocks(cnt * bins_out), dim3(256), 0, ctx->stream, (const CqtCplx<T>*)rs->spec_in.p, (CqtCplx<T>*)rs->spec_out.p, cnt, bins_in,
                           bins_out, n_copy, real_last, k_mid, 1.0 / k_sigma, (T)gain);
        LRA_TRY(get_rocfft_plan(*inv, ctx, rocfft_transform_type_real_inverse, dtype, (int)fft_out, cnt, &plan));
        void* ib2[1] = {rs->spec_out.p};
        void* ob2[1] = {rs->time_out.p};
        LRA_FFT(rocfft_execute(plan, ib2, ob2, inv->info));
        hipLaunchKernelGGL(repitch_rows_kernel<T>, blocks(cnt * n_out), dim3(256), 0, ctx->stream, (const T*)rs->time_out.p, out + c0 * n_out, cnt, n_out, fft_out, n_out);
        LRA_HIP(hipGetLastError());
    }
    LRA_TRY(scratch_release(rs->order, ctx->stream));
    LRA_TRY(scratch_release(*fwd, ctx->stream));  // (an evicted plan is destroyed behind its last use: get_rocfft_plan)
    LRA_TRY(scratch_release(*inv, ctx->stream));
    return rs->trim(ctx->stream, ctx->on_side || ctx->side_used);
}

template <class T> int resample_fft_run(lra_ctx* ctx, const T* x, T* out, long long batch, long long n_in, long long n_out, double gain, int dtype) {
    if (!ctx->rs_fft) ctx->rs_fft = new ResampleFft();
    ResampleFft* rs = ctx->rs_fft;
    const long long bins_in = n_in / 2 + 1, bins_out = n_out / 2 + 1;
    // clips per pass: both spectra of a pass within ~1 GB
    long long per_pass = (1LL << 30) / ((bins_in + bins_out) * (long long)sizeof(cx<T>));
    if (per_pass < 1) per_pass = 1;
    if (per_pass > batch) per_pass = batch;
    LRA_TRY(rs->spec_in.ensure((size_t)per_pass * bins_in * sizeof(cx<T>)));
    LRA_TRY(rs->spec_out.ensure((size_t)per_pass * bins_out * sizeof(cx<T>)));
    const long long N = n_out < n_in ? n_out : n_in;
    const long long n_copy = N / 2 + 1;
    const long long shared = (N % 2 == 0 && n_in != n_out) ? N / 2 : -1;
    const T factor = n_out < n_in ? (T)2 : (T)0.5;
    const long long real_last = n_out % 2 == 0 ? n_out / 2 : -1;
    FftPlanCache* fwd = rs->get((int)rocfft_transform_type_real_forward, dtype, n_in);
    FftPlanCache* inv = rs->get((int)rocfft_transform_type_real_inverse, dtype, n_out);
    LRA_TRY(scratch_acquire(rs->order, ctx->stream));
    for (long long c0 = 0; c0 < batch; c0 += per_pass) {
        const long long cnt = batch - c0 < per_pass ? batch - c0 : per_pass;
        rocfft_plan plan;
        LRA_TRY(get_rocfft_plan(*fwd, ctx, rocfft_transform_type_real_forward, dtype, (int)n_in, cnt, &plan));
        void* ib[1] = {(void*)(x + c0 * n_in)};
        void* ob[1] = {rs->spec_in.p};
        LRA_FFT(rocfft_execute(plan, ib, ob, fwd->info));
        const long long count = cnt * bins_out;
        hipLaunchKernelGGL(resample_spectrum_kernel<T>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, (const CqtCplx<T>*)rs->spec_in.p, (CqtCplx<T>*)rs->spec_out.p, cnt,
                           bins_in, bins_out, n_copy, shared, factor, real_last, (T)gain);
        LRA_HIP(hipGetLastError());
        LRA_TRY(get_rocfft_plan(*inv, ctx, rocfft_transform_type_real_inverse, dtype, (int)n_out, cnt, &plan));
        void* ib2[1] = {rs->spec_out.p};
        void* ob2[1] = {(void*)(out + c0 * n_out)};
        LRA_FFT(rocfft_execute(plan, ib2, ob2, inv->info));
    }
    LRA_TRY(scratch_release(rs->order, ctx->stream));
    LRA_TRY(scratch_release(*fwd, ctx->stream));
    LRA_TRY(scratch_release(*inv, ctx->stream));
    return rs->trim(ctx->stream, ctx->on_side || ctx->side_used);
}
}  // namespace

extern "C" {

int lra_resample_band_exec(lra_ctx* ctx, const void* x, void* out, int64_t batch, int64_t n_in, int64_t n_out, int64_t fft_in, int64_t fft_out, double k_mid, double k_sigma, double gain,
                           int dtype) {
    LRA_BIND(ctx);
    if (batch <= 0 || n_out <= 0) return LRA_OK;
    if (n_in <= 0) return fail(LRA_EINVAL, "resample_band: empty input");
    if (!x || !out) return fail(LRA_EINVAL, "null data pointer");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "resample_band: dtype must be LRA_F32 or LRA_F64");
    if (fft_in < n_in || fft_out < n_out || fft_in > 0x7fffffffLL || fft_out > 0x7fffffffLL) return fail(LRA_EINVAL, "resample_band: transform lengths must cover the signals and stay below 2^31");
    if (!(k_sigma > 0) || !(k_mid > 0)) return fail(LRA_EINVAL, "resample_band: the roll-off needs a positive centre and width");
    if (dtype == LRA_F64) return resample_shaped_run<double>(ctx, (const double*)x, (double*)out, batch, n_in, n_out, fft_in, fft_out, k_mid, k_sigma, gain / (double)fft_in, dtype);
    return resample_shaped_run<float>(ctx, (const float*)x, (float*)out, batch, n_in, n_out, fft_in, fft_out, k_mid, k_sigma, gain / (double)fft_in, dtype);
}

int lra_resample_fft_exec(lra_ctx* ctx, const void* x, void* out, int64_t batch, int64_t n_in, int64_t n_out, double gain, int dtype) {
    LRA_BIND(ctx);
    if (batch <= 0 || n_out <= 0) return LRA_OK;
    if (n_in <= 0) return fail(LRA_EINVAL, "resample_fft: empty input");
    if (!x || !out) return fail(LRA_EINVAL, "null data pointer");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "resample_fft: dtype must be LRA_F32 or LRA_F64");
    if (n_in > 0x7fffffffLL || n_out > 0x7fffffffLL) return fail(LRA_EINVAL, "resample_fft: signal too long for one transform");
    if (dtype == LRA_F64) return resample_fft_run<double>(ctx, (const double*)x, (double*)out, batch, n_in, n_out, gain / (double)n_in, dtype);
    return resample_fft_run<float>(ctx, (const float*)x, (float*)out, batch, n_in, n_out, gain / (double)n_in, dtype);
}

int lra_cqt_project_exec(lra_ctx* ctx, const void* D, void* out, const void* row_ptr, const void* col, const void* val, const void* sqrt_len, int64_t batch, int64_t frames_in, int n_bins,
                         int64_t n_frames, int n_total, int bin0, int row0, int n_rows, int dtype) {
    LRA_BIND(ctx);
    if (n_bins < 1 || n_total < 1 || bin0 < 0 || row0 < 0 || n_rows < 0 || bin0 + n_rows > n_total || n_frames > frames_in)
        return fail(LRA_EINVAL, "cqt_project: the octave's rows must fit the stacked result and its frames the STFT's");
    if (batch <= 0 || n_frames <= 0 || n_rows == 0) return LRA_OK;
    if (!D || !out || !row_ptr || !col || !val) return fail(LRA_EINVAL, "null data pointer");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "cqt_project: dtype must be LRA_F32 or LRA_F64");
    const long long count = (long long)batch * n_frames * n_rows;
    if ((count + 255) / 256 > 0x7fffffffLL) return fail(LRA_EINVAL, "cqt_project: array too large for one launch");
    const unsigned grid = (unsigned)((count + 255) / 256);
    if (dtype == LRA_F64)
        hipLaunchKernelGGL(cqt_project_kernel<double>, dim3(grid), dim3(256), 0, ctx->stream, (const CqtCplx<double>*)D, (CqtCplx<double>*)out, (const int*)row_ptr, (const int*)col,
                           (const CqtCplx<double>*)val, (const double*)sqrt_len, (long long)batch, (long long)frames_in, n_bins, (long long)n_frames, n_total, bin0, row0, n_rows);
    else
        hipLaunchKernelGGL(cqt_project_kernel<float>, dim3(grid), dim3(256), 0, ctx->stream, (const CqtCplx<float>*)D, (CqtCplx<float>*)out, (const int*)row_ptr, (const int*)col,
                           (const CqtCplx<float>*)val, (const double*)sqrt_len, (long long)batch, (long long)frames_in, n_bins, (long long)n_frames, n_total, bin0, row0, n_rows);
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

int lra_cqt_octave_supported(int n_fft) { return mixed::in_cqt_size_list(n_fft) ? 1 : 0; }

int lra_cqt_octave_exec(lra_ctx* ctx, const void* y, int64_t batch, int64_t n, int64_t y_stride, int n_fft, int hop, int pad_mode, const void* row_ptr, const void* col, const void* val,
                        const void* sqrt_len, void* out, int64_t n_frames, int n_total, int bin0, int row0, int n_rows, int dtype) {
    LRA_BIND(ctx);
    if (!mixed::in_cqt_size_list(n_fft)) return fail(LRA_EINVAL, "cqt_octave: n_fft must be a power of two in [32, 4096] (see lra_cqt_octave_supported)");
    if (hop < 1 || pad_mode < LRA_PAD_CONSTANT || pad_mode > LRA_PAD_SYMMETRIC) return fail(LRA_EINVAL, "cqt_octave: bad hop or pad mode");
    if (n_total < 1 || bin0 < 0 || row0 < 0 || n_rows < 0 || bin0 + n_rows > n_total) return fail(LRA_EINVAL, "cqt_octave: the octave's rows must fit the stacked result");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "cqt_octave: dtype must be LRA_F32 or LRA_F64");
    if (batch <= 0 || n_frames <= 0 || n_rows == 0) return LRA_OK;
    if (!y || !out || !row_ptr || !col || !val) return fail(LRA_EINVAL, "null data pointer");
    if (n_frames > 1 + n / hop) return fail(LRA_EINVAL, "cqt_octave: more frames than the centred signal has");
    if (n_frames > 0x7fffffffLL / 4) return fail(LRA_EINVAL, "too many frames per clip");
    const void *tw_m = nullptr, *tw_n = nullptr;
    LRA_TRY(ctx_twiddles(ctx, n_fft, dtype, &tw_m, &tw_n));
    const int F = mixed::cqt_frames_per_group_of(n_fft, dtype == LRA_F64 ? 8 : 4);
    auto fill = [&](auto& a, auto tag) {
        using T = decltype(tag);
        a.y = (const T*)y; a.y_stride = y_stride; a.n = n; a.hop = hop; a.pad = n_fft / 2; a.pad_mode = pad_mode;
        a.tw_m = (const mixed::cpx<T>*)tw_m; a.tw_n = (const mixed::cpx<T>*)tw_n;
        a.row_ptr = (const int*)row_ptr; a.col = (const int*)col; a.val = (const mixed::cpx<T>*)val; a.sqrt_len = (const double*)sqrt_len;
        a.out = (mixed::cpx<T>*)out; a.n_frames = (int)n_frames; a.n_total = n_total; a.bin0 = bin0; a.row0 = row0; a.n_rows = n_rows;
        a.groups_per_clip = (int)((n_frames + F - 1) / F);
        a.nonfinite_flag = ctx->d_flag;
    };
    hipError_t e;
    if (dtype == LRA_F64) {
        mixed::CqtArgs<double> a = mixed::CqtArgs<double>();
        fill(a, double());
        e = mixed::launch_cqt_f64(n_fft, a, batch, ctx->stream);
    } else {
        mixed::CqtArgs<float> a = mixed::CqtArgs<float>();
        fill(a, float());
        e = mixed::launch_cqt_f32(n_fft, a, batch, ctx->stream);
    }
    if (e != hipSuccess) return fail(LRA_EHIP, std::string("cqt octave kernel launch: ") + hipGetErrorString(e));
    return LRA_OK;
}

}  // extern "C"

namespace {
// octaves [i0, i1) of one transform -- same frame length, each on its own (already decimated) signal ys[i] -- in ONE launch (mixed_cqt_multi_kernel)
template <class T>
int cqt_octaves_merged(lra_ctx* ctx, const lra_cqt_octave* octaves, const char* const* ys, int i0, int i1, int64_t batch, int pad_mode, const double* sqrt_len, void* out, int64_t n_frames,
                       int n_total, int dtype) {
    const int n_fft = octaves[i0].n_fft;
    const void *tw_m = nullptr, *tw_n = nullptr;
    LRA_TRY(ctx_twiddles(ctx, n_fft, dtype, &tw_m, &tw_n));
    const int F = mixed::cqt_frames_per_group_of(n_fft, (int)sizeof(T));
    mixed::CqtMultiArgs<T> m = mixed::CqtMultiArgs<T>();
    m.n_oct = 0;
    const int groups = (int)((n_frames + F - 1) / F);
    if ((long long)batch * groups > 0x7fffffffLL) return fail(LRA_EINVAL, "cqt: too many workgroups");
    m.blocks_per_octave = (unsigned)(batch * groups);
    for (int i = i0; i < i1; ++i) {
        const lra_cqt_octave& o = octaves[i];
        if (o.n_rows == 0) continue;
        if (o.hop < 1 || o.bin0 < 0 || o.row0 < 0 || o.n_rows < 0 || o.bin0 + o.n_rows > n_total) return fail(LRA_EINVAL, "cqt_octave: the octave's rows must fit the stacked result");
        if (!o.row_ptr || !o.col || !o.val) return fail(LRA_EINVAL, "null data pointer");
        if (n_frames > 1 + o.n / o.hop) return fail(LRA_EINVAL, "cqt_octave: more frames than the centred signal has");
        mixed::CqtArgs<T>& a = m.oct[m.n_oct++];
        a.y = (const T*)ys[i]; a.y_stride = o.n; a.n = o.n; a.hop = o.hop; a.pad = n_fft / 2; a.pad_mode = pad_mode;
        a.tw_m = (const mixed::cpx<T>*)tw_m; a.tw_n = (const mixed::cpx<T>*)tw_n;
        a.row_ptr = (const int*)o.row_ptr; a.col = (const int*)o.col; a.val = (const mixed::cpx<T>*)o.val; a.sqrt_len = sqrt_len ? sqrt_len + o.bin0 : nullptr;
        a.out = (mixed::cpx<T>*)out; a.n_frames = (int)n_frames; a.n_total = n_total; a.bin0 = o.bin0; a.row0 = o.row0; a.n_rows = o.n_rows;
        a.groups_per_clip = groups;
        a.nonfinite_flag = ctx->d_flag;
    }
    if (m.n_oct == 0) return LRA_OK;
    hipError_t e;
    if constexpr (sizeof(T) == 8) e = mixed::launch_cqt_multi_f64(n_fft, m, ctx->stream);
    else e = mixed::launch_cqt_multi_f32(n_fft, m, ctx->stream);
    if (e != hipSuccess) return fail(LRA_EHIP, std::string("cqt merged octave kernel launch: ") + hipGetErrorString(e));
    return LRA_OK;
}
}  // namespace

extern "C" {

int lra_cqt_recursion_exec(lra_ctx* ctx, const void* y, int64_t batch, const lra_cqt_octave* octaves, int n_octaves, int pad_mode, const void* sqrt_len, void* out, int64_t n_frames,
                           int n_total, const void* taps, int n_taps, int first, void* scratch, int64_t scratch_bytes, int overlap, int dtype) {
    if (!ctx) return fail(LRA_EINVAL, "null context");
    if (n_octaves < 0 || (n_octaves > 0 && !octaves)) return fail(LRA_EINVAL, "cqt_recursion: null octave list");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "cqt_recursion: dtype must be LRA_F32 or LRA_F64");
    // (checked here once, for every path below -- the merged-octave launches do not go through lra_cqt_octave_exec's own checks)
    if (pad_mode < PAD_CONSTANT || pad_mode > PAD_SYMMETRIC) return fail(LRA_EINVAL, "cqt_recursion: unknown pad mode");
    if (n_total < 1) return fail(LRA_EINVAL, "cqt_recursion: n_total must be at least 1");
    if (batch > 0 && n_frames > 0 && n_octaves > 0 && (!y || !out)) return fail(LRA_EINVAL, "cqt_recursion: null data pointer");
    for (int i = 0; i < n_octaves; ++i) {
        const lra_cqt_octave& o = octaves[i];
        if (o.n_rows < 0 || o.bin0 < 0 || o.row0 < 0 || o.bin0 + o.n_rows > n_total || o.hop < 1 || o.n < 0) return fail(LRA_EINVAL, "cqt_recursion: an octave's rows must fit the stacked result");
        if (o.n_rows > 0 && (!o.row_ptr || !o.col || !o.val)) return fail(LRA_EINVAL, "cqt_recursion: null basis table");
    }
    const int64_t es = dtype == LRA_F64 ? 8 : 4;
    // the decimated signals live side by side in `scratch` (each until the call's join: its octave transform runs on the side stream)
    int64_t need = 0;
    for (int i = 0; i + 1 < n_octaves; ++i)
        if (octaves[i].halve) {
            if (octaves[i + 1].n != (octaves[i].n + 1) / 2) return fail(LRA_EINVAL, "cqt_recursion: a halved octave has ceil(n / 2) samples");
            need += ((batch * octaves[i + 1].n * es + 255) / 256) * 256;
        } else if (octaves[i + 1].n != octaves[i].n) {
            return fail(LRA_EINVAL, "cqt_recursion: octaves without a halving in between share their signal");
        }
    if (need > scratch_bytes || (need > 0 && (!scratch || !taps))) return fail(LRA_EINVAL, "cqt_recursion: scratch too small / null");
    for (int i = 0; i < n_octaves; ++i)
        if (!lra_cqt_octave_supported(octaves[i].n_fft)) return fail(LRA_EINVAL, "cqt_recursion: frame length outside the fused octave kernel's list");
    const char* cur = (const char*)y;
    char* next = (char*)scratch;
    const double sc = std::sqrt(0.5);
    const double* sl = (const double*)sqrt_len;
    int rc = LRA_OK;
    bool forked = false;
    if (overlap && ctx->opt_cqt_merge && n_octaves >= 3 && n_octaves <= 1 + mixed::kCqtMaxMerged && n_frames > 0 && batch > 0 && n_frames <= 0x7fffffffLL / 4) {
        // Merged form: the first octave on the side stream beside the chain of halvings, then every further octave in one launch per run of equal frame
        // lengths (their decimated signals all exist by then): the octaves' latency-bound launches overlap instead of queueing up on the side stream.
        LRA_BIND(ctx);
        std::vector<const char*> ys((size_t)n_octaves);
        ys[0] = cur;
        rc = lra_ctx_side(ctx, LRA_SIDE_FORK);
        if (rc == LRA_OK) {
            const lra_cqt_octave& o = octaves[0];
            rc = lra_cqt_octave_exec(ctx, cur, batch, o.n, o.n, o.n_fft, o.hop, pad_mode, o.row_ptr, o.col, o.val, sl ? sl + o.bin0 : nullptr, out, n_frames, n_total, o.bin0, o.row0, o.n_rows, dtype);
            const int rb = lra_ctx_side(ctx, LRA_SIDE_BACK);
            if (rc == LRA_OK) rc = rb;
        }
        // Round 6: with five or more octaves, octaves 1 and 2 go out in a launch of their own on the side stream as soon as their signals exist, beside the
        // remaining (short) halvings, which cannot fill the chip; the rest follows the chain as before (cqt_merge = 2: everything behind the chain).
        int early_end = (ctx->opt_cqt_merge == 1 && n_octaves >= 5) ? std::min(3, n_octaves - 1) : 1;  // one past the last early octave
        for (int i = 2; i < early_end; ++i)
            if (octaves[i].n_fft != octaves[1].n_fft) early_end = 1;  // (one launch serves one frame length)
        for (int i = 0; i + 1 < n_octaves && rc == LRA_OK; ++i) {
            if (octaves[i].halve) {
                rc = lra_fir_decimate_exec(ctx, cur, next, batch, octaves[i].n, octaves[i + 1].n, taps, n_taps, 2, first, sc, 1.0, dtype);
                cur = next;
                next += ((batch * octaves[i + 1].n * es + 255) / 256) * 256;
            }
            ys[(size_t)i + 1] = cur;
            if (rc == LRA_OK && early_end > 1 && i + 2 == early_end) {
                rc = lra_ctx_side(ctx, LRA_SIDE_FORK);
                if (rc == LRA_OK) {
                    rc = dtype == LRA_F64 ? cqt_octaves_merged<double>(ctx, octaves, ys.data(), 1, early_end, batch, pad_mode, sl, out, n_frames, n_total, dtype)
                                          : cqt_octaves_merged<float>(ctx, octaves, ys.data(), 1, early_end, batch, pad_mode, sl, out, n_frames, n_total, dtype);
                    const int rb = lra_ctx_side(ctx, LRA_SIDE_BACK);
                    if (rc == LRA_OK) rc = rb;
                }
            }
        }
        for (int i0 = early_end; i0 < n_octaves && rc == LRA_OK;) {
            int i1 = i0 + 1;
            while (i1 < n_octaves && octaves[i1].n_fft == octaves[i0].n_fft) ++i1;
            rc = dtype == LRA_F64 ? cqt_octaves_merged<double>(ctx, octaves, ys.data(), i0, i1, batch, pad_mode, sl, out, n_frames, n_total, dtype)
                                  : cqt_octaves_merged<float>(ctx, octaves, ys.data(), i0, i1, batch, pad_mode, sl, out, n_frames, n_total, dtype);
            i0 = i1;
        }
        const int rj = lra_ctx_side(ctx, rc == LRA_OK ? LRA_SIDE_JOIN : LRA_SIDE_END);
        return rc == LRA_OK ? rj : rc;
    }
    for (int i = 0; i < n_octaves && rc == LRA_OK; ++i) {
        const lra_cqt_octave& o = octaves[i];
        // the octave's transform on the side stream (behind the halving that made its signal), the next halving on the main stream
        if (overlap) { rc = lra_ctx_side(ctx, LRA_SIDE_FORK); forked = rc == LRA_OK; }
        if (rc == LRA_OK)
            rc = lra_cqt_octave_exec(ctx, cur, batch, o.n, o.n, o.n_fft, o.hop, pad_mode, o.row_ptr, o.col, o.val, sl ? sl + o.bin0 : nullptr, out, n_frames, n_total, o.bin0, o.row0, o.n_rows, dtype);
        if (forked) {
            const int rb = lra_ctx_side(ctx, LRA_SIDE_BACK);
            forked = false;
            if (rc == LRA_OK) rc = rb;
        }
        if (rc == LRA_OK && o.halve && i + 1 < n_octaves) {
            rc = lra_fir_decimate_exec(ctx, cur, next, batch, o.n, octaves[i + 1].n, taps, n_taps, 2, first, sc, 1.0, dtype);
            cur = next;
            next += ((batch * octaves[i + 1].n * es + 255) / 256) * 256;
        }
    }
    if (overlap) {
        const int rj = lra_ctx_side(ctx, rc == LRA_OK ? LRA_SIDE_JOIN : LRA_SIDE_END);
        if (rc == LRA_OK) rc = rj;
    }
    return rc;
}

int lra_magnitude_exec(lra_ctx* ctx, const void* D, void* mag, int64_t count, int dtype) {
    LRA_BIND(ctx);
    if (count <= 0) return LRA_OK;
    if (!D || !mag) return fail(LRA_EINVAL, "null data pointer");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "magnitude: dtype must be LRA_F32 or LRA_F64");
    if ((count + 255) / 256 > 0x7fffffffLL) return fail(LRA_EINVAL, "magnitude: array too large for one launch");
    const unsigned grid = (unsigned)((count + 255) / 256);
    if (dtype == LRA_F64)
        hipLaunchKernelGGL(magnitude_kernel<double>, dim3(grid), dim3(256), 0, ctx->stream, (const HpssCplx<double>*)D, (double*)mag, (long long)count);
    else
        hipLaunchKernelGGL(magnitude_kernel<float>, dim3(grid), dim3(256), 0, ctx->stream, (const HpssCplx<float>*)D, (float*)mag, (long long)count);
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

int lra_magphase_exec(lra_ctx* ctx, const void* D, int is_complex, void* mag, void* phase, int64_t count, double power, int dtype) {
    LRA_BIND(ctx);
    if (count <= 0) return LRA_OK;
    if (!D || !mag || !phase) return fail(LRA_EINVAL, "null data pointer");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "magphase: dtype must be LRA_F32 or LRA_F64");
    if ((count + 255) / 256 > 0x7fffffffLL) return fail(LRA_EINVAL, "magphase: array too large for one launch");
    const unsigned grid = (unsigned)((count + 255) / 256);
    if (dtype == LRA_F64)
        hipLaunchKernelGGL(magphase_kernel<double>, dim3(grid), dim3(256), 0, ctx->stream, D, is_complex ? 1 : 0, (double*)mag, (HpssCplx<double>*)phase, (long long)count, power);
    else
        hipLaunchKernelGGL(magphase_kernel<float>, dim3(grid), dim3(256), 0, ctx->stream, D, is_complex ? 1 : 0, (float*)mag, (HpssCplx<float>*)phase, (long long)count, (float)power);
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

int lra_hpss_exec(lra_ctx* ctx, const void* mag, const void* D, void* out_h, void* out_p, int64_t batch, int64_t n_frames, int n_bins, int win_harm, int win_perc, double power,
                  double margin_harm, double margin_perc, int want_mask, int dtype) {
    LRA_BIND(ctx);
    if (win_harm < 1 || win_perc < 1) return fail(LRA_EINVAL, "hpss: kernel sizes must be positive");
    if (margin_harm < 1 || margin_perc < 1) return fail(LRA_EINVAL, "Margins must be >= 1.0. A typical range is between 1 and 10.");
    if (!(power > 0)) return fail(LRA_EINVAL, "power must be strictly positive");
    if (batch <= 0 || n_frames <= 0 || n_bins <= 0) return LRA_OK;
    if (!mag || !out_h || !out_p) return fail(LRA_EINVAL, "null data pointer");
    if (dtype != LRA_F32 && dtype != LRA_F64) return fail(LRA_EINVAL, "hpss: dtype must be LRA_F32 or LRA_F64");
    const long long count = (long long)batch * n_frames * n_bins;
    if ((count + 255) / 256 > 0x7fffffffLL) return fail(LRA_EINVAL, "hpss: array too large for one launch");
    HpssArgs a;
    a.batch = batch;
    a.n_frames = n_frames;
    a.n_bins = n_bins;
    a.win_harm = win_harm;
    a.win_perc = win_perc;
    a.hard = std::isinf(power) ? 1 : 0;
    a.power = a.hard ? 1.0 : power;
    a.margin_harm = margin_harm;
    a.margin_perc = margin_perc;
    a.want_mask = want_mask ? 1 : 0;
    const unsigned grid = (unsigned)((count + 255) / 256);
    if (dtype == LRA_F64) hpss_launch<double>(ctx, mag, D, out_h, out_p, a, grid);
    else hpss_launch<float>(ctx, mag, D, out_h, out_p, a, grid);
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

int lra_dct_exec(lra_ctx* ctx, const void* S, void* out, int64_t batch, int n_in, int n_out, int64_t n_frames, int dtype, const void* basis, const void* lift, int fuse_db, double amin,
                 double ref_scalar, const void* ref_items, const void* item_max, int use_top_db, double top_db) {
    LRA_BIND(ctx);
    if (batch <= 0 || n_frames <= 0 || n_out <= 0) return LRA_OK;
    if (!S || !out || !basis || !lift) return fail(LRA_EINVAL, "null data pointer");
    if (n_in <= 0) return fail(LRA_EINVAL, "empty band axis");
    if (fuse_db && !(amin > 0)) return fail(LRA_EINVAL, "amin must be strictly positive");
    if (fuse_db && use_top_db && (top_db < 0 || !item_max)) return fail(LRA_EINVAL, "top_db must be non-negative and needs the per-item maxima");
    if (dtype == LRA_F64) {
        DbArgs<double> d{amin, ref_scalar, (const double*)ref_items, use_top_db ? (const double*)item_max : nullptr, top_db};
        return fuse_db ? dct_run<double, true>(ctx, (const double*)S, (double*)out, batch, n_in, n_out, n_frames, (const double*)basis, (const double*)lift, d)
                       : dct_run<double, false>(ctx, (const double*)S, (double*)out, batch, n_in, n_out, n_frames, (const double*)basis, (const double*)lift, d);
    }
    DbArgs<float> d{(float)amin, (float)ref_scalar, (const float*)ref_items, use_top_db ? (const float*)item_max : nullptr, (float)top_db};
    return fuse_db ? dct_run<float, true>(ctx, (const float*)S, (float*)out, batch, n_in, n_out, n_frames, (const float*)basis, (const float*)lift, d)
                   : dct_run<float, false>(ctx, (const float*)S, (float*)out, batch, n_in, n_out, n_frames, (const float*)basis, (const float*)lift, d);
}

#ifdef LRA_PHASE_TIMER
// experiments only (probe builds): read and clear the phase timer of lra_kernels.h
int lra_debug_phase_ticks(lra_ctx* ctx, unsigned long long* out16) {
    LRA_BIND(ctx);
    LRA_HIP(hipStreamSynchronize(ctx->stream));
    LRA_HIP(hipMemcpyFromSymbol(out16, HIP_SYMBOL(lra_phase_ticks), 16 * sizeof(unsigned long long)));
    unsigned long long zero[16] = {};
    LRA_HIP(hipMemcpyToSymbol(HIP_SYMBOL(lra_phase_ticks), zero, sizeof(zero)));
    return LRA_OK;
}
#endif

// ---- transpose ----------------------------------------------------------------------------------
// ---- multi-GPU: gather of the sharded result over RCCL / xGMI ---------------------------------------------------
int lra_comm_unique_id(void* id_out) {
    if (!id_out) return fail(LRA_EINVAL, "null id buffer");
    RcclApi* api = rccl_api();
    if (!api) return fail(LRA_ENODEV, "RCCL (librccl.so) is not available");
    const int rc = api->GetUniqueId(id_out);
    return rc == 0 ? LRA_OK : rccl_fail(api, "ncclGetUniqueId", rc);
}

int lra_comm_init(lra_ctx* ctx, int rank, int n_ranks, const void* id, lra_comm** out) {
    LRA_BIND(ctx);
    if (!out || !id) return fail(LRA_EINVAL, "null argument");
    *out = nullptr;
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(LRA_EINVAL, "bad rank / n_ranks");
    RcclApi* api = rccl_api();
    if (!api) return fail(LRA_ENODEV, "RCCL (librccl.so) is not available");
    RcclApi::Id uid;
    std::memcpy(uid.b, id, sizeof(uid.b));
    void* comm = nullptr;
    const int rc = api->CommInitRank(&comm, n_ranks, uid, rank);  // the communicator binds to the calling thread's current device = ctx's (LRA_BIND)
    if (rc != 0) return rccl_fail(api, "ncclCommInitRank", rc);
    lra_comm* c = new lra_comm();
    c->ctx = ctx;
    c->nccl = comm;
    c->rank = rank;
    c->n_ranks = n_ranks;
    *out = c;
    return LRA_OK;
}

int lra_comm_allgather(lra_comm* comm, const void* send_dev, void* recv_dev, size_t bytes_per_rank) {
    if (!comm) return fail(LRA_EINVAL, "null communicator");
    LRA_BIND(comm->ctx);
    if (!bytes_per_rank) return LRA_OK;
    if (!send_dev || !recv_dev) return fail(LRA_EINVAL, "null data pointer");
    RcclApi* api = rccl_api();
    if (!api) return fail(LRA_ENODEV, "RCCL (librccl.so) is not available");
    const int rc = api->AllGather(send_dev, recv_dev, bytes_per_rank, /* ncclInt8 */ 0, comm->nccl, comm->ctx->stream);
    return rc == 0 ? LRA_OK : rccl_fail(api, "ncclAllGather", rc);
}

int lra_comm_allgatherv(lra_comm* comm, const void* send_dev, void* recv_dev, const size_t* bytes_per_rank, const size_t* recv_offsets) {
    if (!comm) return fail(LRA_EINVAL, "null communicator");
    LRA_BIND(comm->ctx);
    if (!bytes_per_rank || !recv_offsets) return fail(LRA_EINVAL, "null size / offset table");
    if (!recv_dev) return fail(LRA_EINVAL, "null data pointer");
    RcclApi* api = rccl_api();
    if (!api) return fail(LRA_ENODEV, "RCCL (librccl.so) is not available");
    if (!api->Broadcast || !api->GroupStart || !api->GroupEnd) return fail(LRA_ENODEV, "this RCCL has no ncclBroadcast / ncclGroupStart / ncclGroupEnd");
    if (bytes_per_rank[comm->rank] && !send_dev) return fail(LRA_EINVAL, "null data pointer");
    // unequal shards: every rank broadcasts its own piece into its slice of the full buffer, all of them inside ONE group (one fused operation on the wire)
    int rc = api->GroupStart();
    if (rc != 0) return rccl_fail(api, "ncclGroupStart", rc);
    int first_bad = 0;
    for (int r = 0; r < comm->n_ranks; ++r) {
        if (!bytes_per_rank[r]) continue;
        char* slice = (char*)recv_dev + recv_offsets[r];
        const int e = api->Broadcast(r == comm->rank ? send_dev : slice, slice, bytes_per_rank[r], /* ncclInt8 */ 0, r, comm->nccl, comm->ctx->stream);
        if (e != 0 && !first_bad) first_bad = e;
    }
    rc = api->GroupEnd();
    if (first_bad) return rccl_fail(api, "ncclBroadcast", first_bad);
    return rc == 0 ? LRA_OK : rccl_fail(api, "ncclGroupEnd", rc);
}

void lra_comm_destroy(lra_comm* comm) {
    if (!comm) return;
    RcclApi* api = rccl_api();
    if (api && comm->nccl) (void)api->CommDestroy(comm->nccl);
    delete comm;
}

int lra_probe_stream(lra_ctx* ctx, int direction, const void* in, void* out, int64_t batch, int64_t rows_per_clip, int n_fft, int hop, int64_t clip_samples, int strip_rows,
                     int waves_per_cu) {
    return lra_probe_stream_pitched(ctx, direction, in, out, batch, rows_per_clip, n_fft, hop, clip_samples, strip_rows, waves_per_cu, 0, 8);
}

int lra_probe_stream_pitched(lra_ctx* ctx, int direction, const void* in, void* out, int64_t batch, int64_t rows_per_clip, int n_fft, int hop, int64_t clip_samples,
                             int strip_rows, int waves_per_cu, int64_t row_pitch_bytes, int piece_bytes) {
    LRA_BIND(ctx);
    if (batch <= 0 || rows_per_clip <= 0) return LRA_OK;
    if (!in || !out) return fail(LRA_EINVAL, "null data pointer");
    const int M = n_fft / 2;
    if (n_fft < 256 || n_fft > 2048 || M % 128 != 0) return fail(LRA_EINVAL, "probe: n_fft must be 256 ... 2048, a multiple of 256");
    if (hop <= 0 || hop > 1024 || hop % 128 != 0) return fail(LRA_EINVAL, "probe: hop must be a multiple of 128, at most 1024");
    if (direction != 0 && direction != 1) return fail(LRA_EINVAL, "probe: direction 0 (forward stream) or 1 (inverse stream)");
    if (rows_per_clip > 0x7fffffffLL || batch > 0x7fffffffLL) return fail(LRA_EINVAL, "probe: too many rows");
    ProbeArgs a;
    a.in = (const char*)in;
    a.out = (char*)out;
    a.clip_in_bytes = (long long)clip_samples * 4;
    a.rows_per_clip = (int)rows_per_clip;
    a.strip_rows = strip_rows > 0 ? strip_rows : 162;
    a.n_clips = (int)batch;
    a.bins = M + 1;
    a.row_pitch = row_pitch_bytes > 0 ? row_pitch_bytes : (long long)(M + 1) * 8;
    if (a.row_pitch < (long long)(M + 1) * 8 || a.row_pitch % 8 != 0) return fail(LRA_EINVAL, "probe: row pitch must be a multiple of 8 bytes, at least one row");
    if (piece_bytes != 8 && piece_bytes != 16) return fail(LRA_EINVAL, "probe: pieces of 8 or 16 bytes");
    if (piece_bytes == 16 && (a.row_pitch % 16 != 0 || ((size_t)(direction == 0 ? out : in) & 15))) return fail(LRA_EINVAL, "probe: 16-byte pieces need 16-byte aligned rows");
    a.hop_bytes = hop * 4;
    const long long pcm_rows = clip_samples / hop;
    a.pcm_rows = (int)(pcm_rows < rows_per_clip ? pcm_rows : rows_per_clip);
    const long long strips = (long long)batch * ((rows_per_clip + a.strip_rows - 1) / a.strip_rows);
    const long long grid = (strips + 7) / 8 * 8;
    if (grid > 0x7ffffff0LL) return fail(LRA_EINVAL, "probe: grid too large");
    a.xcd_chunk = ctx->opt_xcd_remap ? (int)(grid / 8) : 0;
    const int wpc = waves_per_cu > 0 ? waves_per_cu : 12;
    const int lds = wpc >= 32 ? 0 : ((160 * 1024 / wpc) & ~255);  // one wave per workgroup: the LDS pad bounds the resident waves per CU
    auto kern = direction == 0 ? (piece_bytes == 16 ? stream_probe_kernel<0, true> : stream_probe_kernel<0, false>)
                               : (piece_bytes == 16 ? stream_probe_kernel<1, true> : stream_probe_kernel<1, false>);
    if (lds > 65536) LRA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64), lds, ctx->stream, a);
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

int lra_probe_stream_window(lra_ctx* ctx, const void* in, void* out, int64_t batch, int64_t rows_per_clip, int n_fft, int hop, int64_t clip_samples, int strip_rows, int waves_per_cu) {
    LRA_BIND(ctx);
    if (batch <= 0 || rows_per_clip <= 0) return LRA_OK;
    if (!in || !out) return fail(LRA_EINVAL, "null data pointer");
    const int M = n_fft / 2;
    if (n_fft < 256 || n_fft > 2048 || M % 128 != 0) return fail(LRA_EINVAL, "probe: n_fft must be 256 ... 2048, a multiple of 256");
    if (hop <= 0 || hop > 1024 || hop % 128 != 0) return fail(LRA_EINVAL, "probe: hop must be a multiple of 128, at most 1024");
    if (strip_rows < 1 || waves_per_cu < 1 || waves_per_cu > 32) return fail(LRA_EINVAL, "probe: strip_rows >= 1, 1 <= waves_per_cu <= 32");
    ProbeArgs a;
    a.in = (const char*)in;
    a.out = (char*)out;
    a.clip_in_bytes = (long long)clip_samples * 4;
    a.rows_per_clip = (int)rows_per_clip;
    a.strip_rows = strip_rows;
    a.n_clips = (int)batch;
    a.bins = M + 1;
    a.row_pitch = (long long)(M + 1) * 8;
    a.hop_bytes = hop * 4;
    const long long pcm_rows = clip_samples / hop;
    a.pcm_rows = (int)(pcm_rows < rows_per_clip ? pcm_rows : rows_per_clip);
    a.xcd_chunk = 0;
    const int n_workers = ctx->n_cu * waves_per_cu;
    const int lds = waves_per_cu >= 32 ? 0 : ((160 * 1024 / waves_per_cu) & ~255);
    if (lds > 65536) LRA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(stream_probe_window_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(stream_probe_window_kernel, dim3((unsigned)n_workers), dim3(64), lds, ctx->stream, a, (long long)batch * rows_per_clip, n_workers);
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

int lra_transpose(lra_ctx* ctx, const void* src, void* dst, int64_t batch, int64_t rows, int64_t cols, int elem_bytes) {
    LRA_BIND(ctx);
    if (batch <= 0 || rows <= 0 || cols <= 0) return LRA_OK;
    if (!src || !dst) return fail(LRA_EINVAL, "null data pointer");
    if (batch > 65535) return fail(LRA_EINVAL, "transpose batch too large");
    dim3 grid((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32), (unsigned)batch), block(32, 8);
    if (grid.y > 65535) return fail(LRA_EINVAL, "transpose rows too large");
    switch (elem_bytes) {
        case 4: hipLaunchKernelGGL(transpose_kernel<uint32_t>, grid, block, 0, ctx->stream, (const uint32_t*)src, (uint32_t*)dst, (long long)rows, (long long)cols); break;
        case 8: hipLaunchKernelGGL(transpose_kernel<uint64_t>, grid, block, 0, ctx->stream, (const uint64_t*)src, (uint64_t*)dst, (long long)rows, (long long)cols); break;
        case 16: hipLaunchKernelGGL(transpose_kernel<double2>, grid, block, 0, ctx->stream, (const double2*)src, (double2*)dst, (long long)rows, (long long)cols); break;
        default: return fail(LRA_EINVAL, "elem_bytes must be 4, 8 or 16");
    }
    LRA_HIP(hipGetLastError());
    return LRA_OK;
}

}  // extern "C"
