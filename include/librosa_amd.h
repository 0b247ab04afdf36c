/* librosa_amd.h -- C ABI of the MI355X (gfx950) implementation of librosa's STFT -> mel (+ ISTFT)
 * hot path.
 *
 * The reference (librosa, pure Python) exposes no C ABI / FFI for this path; its only swap point
 * is scipy.fft's uarray backend at the rfft/irfft call sites (librosa/core/spectrum.py:372,376,
 * 388,566,598), which hands over host float64 blocks of <= 32 frames and is the wrong granularity
 * for a GPU.  The drop-in boundary is therefore librosa's Python function level,
 * and this header is what the Python shim (librosa_amd/, ctypes) binds underneath it.  Every entry
 * point cites the reference code whose arithmetic it replaces.
 *
 * Conventions
 *   - plain C types only; every function returns 0 (LRA_OK) or a negative LRA_E* code, and
 *     lra_last_error() returns the message of the calling thread's last failure;
 *   - every data pointer is a DEVICE pointer unless the parameter is documented as "host";
 *     the caller owns all buffers; the library never frees or reallocates them;
 *   - all work is enqueued on the context's stream (its own, or one adopted with
 *     lra_ctx_set_stream, e.g. PyTorch's current stream); calls are asynchronous with respect to
 *     the host unless documented otherwise;
 *   - device layouts are row-major:  PCM y[batch][n];  spectrum D[batch][n_frames][n_bins]
 *     (n_bins = 1 + n_fft/2, interleaved re/im) -- librosa's (..., n_bins, n_frames) array is a
 *     transposed view of this buffer, exactly like the Fortran-ordered array the reference
 *     allocates (core/spectrum.py:356);  mel M[batch][n_mels][n_frames] (C order, as the
 *     reference's einsum returns, feature/spectral.py:2160).
 */
#ifndef LIBROSA_AMD_H
#define LIBROSA_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRA_OK 0
#define LRA_EINVAL (-1)   /* bad argument (maps to librosa.ParameterError in the shim) */
#define LRA_EHIP (-2)     /* HIP runtime error */
#define LRA_EROCFFT (-3)  /* rocFFT error */
#define LRA_ENODEV (-4)   /* no usable gfx950 device */
#define LRA_ENOMEM (-5)

#define LRA_F32 0 /* float32 PCM  <-> complex64  spectrum (util.dtype_r2c, util/utils.py:2404-2416) */
#define LRA_F64 1 /* float64 PCM  <-> complex128 spectrum */

/* np.pad modes that depend only on edge values (the ones stft supports natively on the device;
 * the shim pre-pads for the exotic ones; "wrap/maximum/mean/median/minimum" are rejected as in
 * core/spectrum.py:253-265). */
#define LRA_PAD_CONSTANT 0
#define LRA_PAD_REFLECT 1
#define LRA_PAD_EDGE 2
#define LRA_PAD_SYMMETRIC 3

typedef struct lra_ctx lra_ctx;
typedef struct lra_event lra_event;
typedef struct lra_stft_plan lra_stft_plan;
typedef struct lra_mel_plan lra_mel_plan;
typedef struct lra_istft_plan lra_istft_plan;

/* ---- library / context ------------------------------------------------------------------ */
const char* lra_last_error(void);
const char* lra_version(void);
int lra_device_count(int* count);
/* One context = one device + one stream + error state.  Fails with LRA_ENODEV when no GPU. */
int lra_ctx_create(int device, lra_ctx** out);
void lra_ctx_destroy(lra_ctx* ctx);
/* Enqueue on an existing hipStream_t, e.g. PyTorch's current stream.  NULL means HIP's default
 * (null) stream -- which is what torch.cuda.current_stream() is unless the caller changed it. */
int lra_ctx_set_stream(lra_ctx* ctx, void* hip_stream);
/* Go back to the context's own (non-blocking) stream. */
int lra_ctx_use_own_stream(lra_ctx* ctx);
/* A second stream of the context for work that may overlap the main chain (the constant-Q recursion: the octave transforms run beside
 * the chain of halvings, librosa/core/constantq.py:1054-1099).  LRA_SIDE_FORK: calls from now on are enqueued on the side stream, behind
 * everything enqueued on the main stream so far; LRA_SIDE_BACK: back to the main stream, which does NOT wait for the side stream;
 * LRA_SIDE_JOIN (from the main stream): the main stream waits for everything enqueued on the side stream.  Buffers used on the side
 * stream must stay alive until a join; LRA_SIDE_END = back (if forked) + join, for error paths.  The two directions use separate
 * events, and every fork its own event out of a ring whose slots are reused only once the side stream is past its wait on them
 * (re-recording one event that the other stream still waits on let that wait slip on ROCm 7.0: a use-after-free in the
 * caller's buffers).  lra_ctx_set_stream / lra_ctx_use_own_stream forget any fork. */
#define LRA_SIDE_FORK 1
#define LRA_SIDE_BACK 2
#define LRA_SIDE_JOIN 3
#define LRA_SIDE_END 4
int lra_ctx_side(lra_ctx* ctx, int mode);
int lra_ctx_sync(lra_ctx* ctx);
/* Tuning knobs: "stft_iters" (frames per slot, 0 = auto), "istft_strip_groups" (frames per strip, 0 = auto),
   "variant" (-1 = auto), "autotune" (1/0).  Kernel-form switches kept for same-box A/B runs (defaults in brackets; DESIGN.md 4.2 / 4.4b / 4.6d say what
   each form is): "v2" [1], "v3" [1: radices 16-16-4 for the complex epilogue; 2: for |X|^p and mel too], "mel_pc" [1: producer / consumer mel kernel; 2: on the
   16-16-4 core], "istft16" [0], "direct" [1], "mixed" [1: fused mixed-radix kernels; 2: the same with the mel band table read through the caches; 0: rocFFT path],
   "mixed_inv_pow2" [1], "mixed_irfft" [1: inverse transform of long mixed-radix frames as one launch in front of the gather kernel; 0: spec_pack + rocFFT C2R],
   "ola4" [1: four samples per thread in the gather kernel], "mixed_pow2_mel" [1: n_fft 128 / 256 with many bands on the flat-index kernel],
   "cqt_merge" [1: octaves 1-2 beside the later halvings; 2: all octaves behind the chain; 0: one launch per octave], "mel_many" [1], "hpss_tile" [1],
   "placement_retry" [4; 0 = off], "pipe_chunk_mb" [128], "pipe_threads" [8], "xcd_remap" [1].  Unknown keys are an error.  The same keys can be preset for
   every context of a process through the environment: LRA_CTX_OPTIONS="key=value,key=value". */
int lra_ctx_set_option(lra_ctx* ctx, const char* key, int value);
int lra_ctx_device_name(lra_ctx* ctx, char* buf, size_t buflen);
/* Device-side half of util.valid_audio (librosa/util/utils.py:294-306): the fused power-of-two STFT
 * kernels raise a sticky flag when a frame's DC bin is not finite, which (barring overflow) happens
 * iff some sample of the frame is NaN/Inf.  reset clears it (async); read syncs the stream. */
int lra_ctx_nonfinite_reset(lra_ctx* ctx);
int lra_ctx_nonfinite_read(lra_ctx* ctx, int* flag);
/* 1 when the plan runs the fused power-of-two kernels (and therefore feeds the flag above). */
int lra_stft_plan_is_fused(const lra_stft_plan* plan);
/* Kernel variant the plan settled on for an epilogue (mode 0 = stft, 1 = spectrogram, 2 = melspectrogram), after the
   first large call timed the candidates (ctx option "autotune", default on; "variant" >= 0 pins one instead):
   -1 = not measured (yet).  Reporting only (bench.py); the reference has no counterpart. */
int lra_stft_plan_tuned_variant(const lra_stft_plan* plan, int mode);
int lra_istft_plan_tuned_variant(const lra_istft_plan* plan);

/* device memory helpers for hosts that do not bring their own allocator (NumPy path of the shim) */
int lra_malloc(lra_ctx* ctx, size_t bytes, void** dptr);
int lra_free(lra_ctx* ctx, void* dptr);
/* Placement-aware allocation of a LARGE, long-lived result buffer of rows (a spectrum: the Fortran-ordered array of core/spectrum.py:356 seen
 * frame-major, `row_bytes` per frame).  Where such a buffer lands in HBM moves the store-bound transforms by up to 15 % on some boxes
 * (profiles/r05_pitch.md); this call builds up to `tries` candidates (ctx option "placement_retry" overrides; 1..8) -- alternately an ordinary hipMalloc
 * block and a range assembled from 64 MiB physical handles mapped in order: which kind lands better differs from box to box -- times the kernels' write
 * stream on each (~1 ms per candidate), keeps the best and releases the rest.  It stops early where two
 * candidates agree within 1.5 % (no lottery on this box) or one matches the best this context has seen.  rows_per_item: rows of one clip (its
 * frames; 0 = no item structure) -- the probe cuts the buffer into per-clip strips of rows exactly as the kernels do, because WHICH rows are written
 * at the same time is what the placement levels depend on.  probe_ms / tried: optional outputs.
 * Free with lra_free_placed only.  bytes >= 4096 rows; row_bytes a multiple of 8, >= 512.
 * Address ranges are never re-used or freed while the context lives (on ROCm 7.0 / gfx950 that leaves other live ranges with stale translations:
 * scripts/vmm_coherence.hip); a context spends at most 4 TiB of address space this way, then the call fails with LRA_ENOMEM and callers allocate normally. */
int lra_malloc_placed(lra_ctx* ctx, size_t bytes, int row_bytes, int64_t rows_per_item, int tries, void** dptr, float* probe_ms, int* tried);
int lra_free_placed(lra_ctx* ctx, void* dptr);
int lra_memset(lra_ctx* ctx, void* dptr, int value, size_t bytes);
int lra_memcpy_h2d(lra_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes); /* synchronous */
int lra_memcpy_d2h(lra_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes); /* synchronous */

/* HIP events on the context's stream (bench.py times the kernels with these) */
int lra_event_create(lra_ctx* ctx, lra_event** out);
void lra_event_destroy(lra_event* ev);
int lra_event_record(lra_event* ev);
int lra_event_elapsed_ms(lra_event* start, lra_event* stop, float* ms); /* syncs on stop */

/* ---- STFT: librosa.stft, librosa/core/spectrum.py:57-391 ------------------------------- */
/* window: host pointer, n_fft reals of `dtype` = pad_center(get_window(window, win_length), n_fft)
 * (core/spectrum.py:243-246), built by the shim with the reference's own scipy call.
 * center != 0 pads n_fft/2 samples each side with pad_mode (core/spectrum.py:252-328).  Power-of-two
 * n_fft in [32, 16384] (f64: 8192) runs the fused LDS-FFT kernels; any other n_fft runs a framing
 * kernel + rocFFT batched R2C. */
int lra_stft_plan_create(lra_ctx* ctx, int n_fft, int hop_length, const void* window_host, int center, int pad_mode, int dtype,
                         lra_stft_plan** out);
void lra_stft_plan_destroy(lra_stft_plan* plan);
/* n_frames = 1 + (n + 2*(n_fft/2)*center - n_fft) / hop  (core/spectrum.py:344-353); LRA_EINVAL when
 * n_fft > n and not centred (core/spectrum.py:330-333). */
int lra_stft_num_frames(const lra_stft_plan* plan, int64_t n, int64_t* n_frames);
/* D[batch][n_frames][n_bins] = rfft(window * frames)  (core/spectrum.py:380-390). */
int lra_stft_exec(lra_stft_plan* plan, const void* y, int64_t batch, int64_t n, int64_t y_stride, void* D);
/* S[batch][n_frames][n_bins] = |stft|**power  (_spectrogram, core/spectrum.py:3000-3013). */
int lra_spectrogram_exec(lra_stft_plan* plan, const void* y, int64_t batch, int64_t n, int64_t y_stride, double power, void* S);
/* The same two results with the rows of consecutive frames `out_frame_stride` ELEMENTS apart (>= n_bins; 0 = n_bins = the calls above):
 * kind 0 = lra_stft_exec, kind 1 = lra_spectrogram_exec.  The array librosa.stft returns is itself a strided view -- (..., n_bins, n_frames)
 * over storage whose fastest axis is the bin axis (core/spectrum.py:356, order="F") -- so a caller may pad each frame's row to a whole
 * number of 128-byte cache lines (1040 complex64 for n_fft = 2048) and present out[..., :n_bins] transposed: every wave-wide store of the
 * kernels then covers whole lines (round 5, profiles/r05_pitch.md).  Only the elements [0, n_bins) of a row are written.  Fused power-of-two
 * plans only (lra_stft_plan_is_fused); LRA_EINVAL otherwise. */
int lra_stft_exec_strided(lra_stft_plan* plan, int kind, const void* y, int64_t batch, int64_t n, int64_t y_stride, double power, void* out, int64_t out_frame_stride);

/* Host-buffer form of the three forward calls (what librosa.stft / _spectrogram / feature.melspectrogram take: NumPy arrays,
 * core/spectrum.py:57-391, :2920-3015, feature/spectral.py:2145-2160).  y_host: [batch] rows of n reals, y_stride elements
 * apart, pageable host memory; out_host: [batch] items of [n_frames][n_bins] complex (kind 0), [n_frames][n_bins] reals
 * (kind 1, |X|**power) or [n_mels][n_frames] reals (kind 2; mel required), out_item_stride reals apart (0 = packed).
 * Clips are moved in stages of ~pipe_chunk_mb (ctx option): host threads copy to / from pinned staging while the previous
 * stage's upload, kernel and download run on their own streams, so the call runs at link rate instead of at the rate of
 * a pageable copy.  Staging and device buffers persist in the context: a streaming caller (librosa.stream blocks ->
 * stft(center=False, out=D), docs/examples/plot_pcen_stream.py:72-74) allocates nothing after its first block.
 * nonfinite (optional): the staging threads also apply util.valid_audio's test (util/utils.py:305: every sample finite) to
 * the samples they copy; *nonfinite != 0 when it failed (the caller raises, the output is then meaningless).
 * Synchronous: out_host is complete on return. */
int lra_stft_exec_host(lra_stft_plan* plan, lra_mel_plan* mel, int kind, const void* y_host, int64_t batch, int64_t n, int64_t y_stride, double power,
                       void* out_host, int64_t out_item_stride, int* nonfinite);

/* ---- mel: librosa.filters.mel (filters.py:116-251) applied as in feature/spectral.py:2158-2160 */
/* basis: host pointer, dense [n_mels][n_bins] reals of `dtype`, built by the shim on the host with
 * the reference's float64 recipe (so it is bit-identical to filters.mel); stored on the device in
 * band form (first/last non-zero column per row; 2018 of 131200 entries at the default config). */
int lra_mel_plan_create(lra_ctx* ctx, int n_mels, int n_bins, const void* basis_host, int dtype, lra_mel_plan** out);
void lra_mel_plan_destroy(lra_mel_plan* plan);
/* Fused feature.melspectrogram(y=...): M[batch][n_mels][n_frames]; the complex spectrum never
 * reaches HBM (feature/spectral.py:2145-2160). */
int lra_melspectrogram_exec(lra_stft_plan* stft, lra_mel_plan* mel, const void* y, int64_t batch, int64_t n, int64_t y_stride, double power,
                            void* M);
/* feature.melspectrogram(S=...): M[b][m][t] = sum_f basis[m][f] * S[b*batch_stride + f*bin_stride + t*frame_stride]. */
int lra_mel_apply_exec(lra_mel_plan* mel, const void* S, int64_t batch, int64_t n_frames, int64_t batch_stride, int64_t bin_stride,
                       int64_t frame_stride, void* M);

/* ---- ISTFT: librosa.istft, librosa/core/spectrum.py:394-626 (+ __overlap_add :629-643) ---- */
int lra_istft_plan_create(lra_ctx* ctx, int n_fft, int hop_length, const void* window_host, int center, int dtype, lra_istft_plan** out);
void lra_istft_plan_destroy(lra_istft_plan* plan);
/* D: [batch] x frames x n_bins with the given element strides (d_frame_stride >= n_bins);
 * frames [0, n_used) are inverse-transformed, windowed and overlap-added in frame order; sample s of
 * the output is padded position s + n_fft/2 (centred) or s; wss (device, [out_len]) is
 * fix_length(window_sumsquare(...)[start:], out_len) computed by the shim exactly as the reference
 * does (core/spectrum.py:606-620); y[batch][out_len] = ola / wss where wss > tiny (:622-624). */
int lra_istft_exec(lra_istft_plan* plan, const void* D, int64_t batch, int64_t d_batch_stride, int64_t d_frame_stride, int64_t n_used,
                   const void* wss, void* y, int64_t out_len, int64_t y_stride);

/* The same transform with the normalisation handed over as FACTORS: norm[s] = 1 / wss[s] where wss[s] > tiny, else 1 (device, [out_len]) --
 * the form the fused kernels consume (y = ola * norm: core/spectrum.py:622-624 as a multiplication, within 1 ulp of the division).  A caller
 * that keeps the envelope of a (window, hop, length) combination around (the Python shim memoises it per context) builds the factors once;
 * lra_istft_exec derives them from `wss` with one small launch per call. */
int lra_istft_exec_norm(lra_istft_plan* plan, const void* D, int64_t batch, int64_t d_batch_stride, int64_t d_frame_stride, int64_t n_used,
                        const void* norm, void* y, int64_t out_len, int64_t y_stride);

/* Host-buffer form (librosa.istft on np.ndarrays): D_host [batch][n_frames][n_bins] complex, packed, pageable; wss_host
 * [out_len] reals; y_host [batch] rows of out_len reals, y_stride apart.  Same staged, overlapped transfer as
 * lra_stft_exec_host. */
int lra_istft_exec_host(lra_istft_plan* plan, const void* D_host, int64_t batch, int64_t n_frames, int64_t n_used, const void* wss_host, void* y_host,
                        int64_t out_len, int64_t y_stride);

/* ---- decibel scaling: librosa.power_to_db / amplitude_to_db, librosa/core/spectrum.py:1735-1883, 1946-2038 ---- */
/* Arrays are [batch][per_item] (the shim flattens the reduced axes -- "auto" = the last two -- into per_item).
 * out_max[b] = max_i |x[b][i]|: the reduction behind ref=np.max and top_db (log_spec.max(axes), :1877-1881). */
int lra_item_absmax_exec(lra_ctx* ctx, const void* x, int64_t batch, int64_t per_item, int dtype, void* out_max);
/* absolute != 0: as above (amplitude_to_db takes np.abs of every input, :2011).  absolute == 0: out_max[b] = max(0, max_i x[b][i]) --
 * power_to_db leaves real input signed (:1855-1859), and every use of the maximum is max(amin, .) with amin > 0. */
int lra_item_max_exec(lra_ctx* ctx, const void* x, int64_t batch, int64_t per_item, int dtype, int absolute, void* out_max);
/* out = 10 log10(max(amin, mag)) - 10 log10(max(amin, ref)), floored at its per-item maximum - top_db (:1873-1881).
 * amplitude != 0: mag = x**2, ref -> ref**2 (amplitude_to_db, :2030-2037; pass amin already squared), else mag = x as it is
 * (complex input has its modulus taken by the caller, :1855-1859; negative real values floor at amin).
 * ref_items (device, [batch]) overrides ref_scalar; item_max (device, [batch], input domain) is read when use_top_db. */
int lra_to_db_exec(lra_ctx* ctx, const void* x, void* out, int64_t batch, int64_t per_item, int dtype, int amplitude, double amin, double ref_scalar,
                   const void* ref_items, const void* item_max, int use_top_db, double top_db);
/* db_to_power: ref * 10**(0.1 x) (:1925); amplitude != 0: db_to_amplitude = db_to_power(x, ref**2)**0.5 (:2082). */
int lra_from_db_exec(lra_ctx* ctx, const void* x, void* out, int64_t count, int dtype, int amplitude, double ref);

/* ---- MFCC: librosa.feature.mfcc, librosa/feature/spectral.py:1843-2019 --------------------------------------------- */
/* out[b][k][t] = lift[k] * sum_m basis[m][k] * f(S[b][m][t]), k < n_out.  basis (device): band-major [n_in][ldc],
 * basis[m][k] = scipy.fft.dct(eye(n_in), axis=0, type, norm)[k][m] (:2005), ldc = n_out rounded up to a multiple of 128, zeros
 * beyond n_out;
 * lift (device, [n_out]): 1 + (lifter/2) sin(pi (k+1) / lifter) or ones (:2008-2015).  fuse_db != 0: f is the decibel
 * scaling of lra_to_db_exec (power domain), so that mfcc(y=...) reads the mel power spectrogram once (:2001). */
int lra_dct_exec(lra_ctx* ctx, const void* S, void* out, int64_t batch, int n_in, int n_out, int64_t n_frames, int dtype, const void* basis, const void* lift,
                 int fuse_db, double amin, double ref_scalar, const void* ref_items, const void* item_max, int use_top_db, double top_db);

/* ---- Griffin-Lim: librosa.griffinlim, librosa/core/spectrum.py:2669-2917 ------------------------------------------- */
/* One phase update over `count` complex values (:2896-2902):
 *   angles = rebuilt - coef * tprev (tprev may be NULL: first iteration);  angles /= |angles| + eps;  angles *= S
 * coef = momentum / (1 + momentum), eps = tiny(angles) (:2830).  normalize == 0: angles = rebuilt * S only (:2847).
 * rebuilt / tprev / angles: complex of `dtype`'s precision, S: real, all in the same element order ([batch][frame][bin] in
 * the shim's loop: lra_istft_exec -> lra_stft_exec -> this, device-resident across iterations); angles may alias rebuilt. */
int lra_griffinlim_update(lra_ctx* ctx, const void* rebuilt, const void* tprev, const void* S, void* angles, int64_t count, int dtype, double coef, double eps,
                          int normalize);

/* Initial estimate (:2832-2847, init="random"): angles = S * exp(2 pi i u), u: device array of float64 uniform draws (the
 * caller's rng.random(S.shape), so that a seed reproduces the reference's stream), in the element order of S / angles. */
int lra_griffinlim_init(lra_ctx* ctx, const void* u, const void* S, void* angles, int64_t count, int dtype);

/* NumPy's default generator on the device (round 5): PCG64 = PCG XSL RR 128/64 with O(log n) jump-ahead per thread, integer arithmetic only, so
 * the stream is np.random.default_rng's bit for bit.  state4 (host) = {state_hi, state_lo, inc_hi, inc_lo}: the two 128-bit integers of
 * Generator.bit_generator.state["state"].  out[i] (device, float64) = draw number offset + i, i.e. rng.random(offset + count)[offset:]. */
int lra_pcg64_random_exec(lra_ctx* ctx, const uint64_t* state4, uint64_t offset, void* out, int64_t count);
/* lra_griffinlim_init with the draws made in place: angles = S * exp(2 pi i u), u = rng.random((batch, n_bins, n_frames)) in THAT element order
 * (the reference's `rng.random(size=S.shape)`, librosa/core/spectrum.py:2832-2847), S / angles in the device layout [batch][frame][bin].
 * The caller advances its host generator by batch * n_bins * n_frames draws (bit_generator.advance) to leave it where the reference would. */
int lra_griffinlim_init_pcg64(lra_ctx* ctx, const uint64_t* state4, const void* S, void* angles, int64_t batch, int n_bins, int64_t n_frames, int dtype);

/* ---- phase vocoder: librosa.phase_vocoder, librosa/core/spectrum.py:1364-1519 (effects.time_stretch, effects.py:464-484) ---- */
/* D: [batch][n_frames][n_bins] complex (device), out: [batch][n_out][n_bins]; t_out_host: n_out fractional input frame times in
 * [0, n_frames) (np.arange(0, n_frames, rate) for a constant rate, :1488).  Phase: running sum of the phase differences of the
 * two input frames around each time (:1491-1507); magnitude: scipy interp1d(kind="linear") of |D| (:1507-1515). */
int lra_phase_vocoder_exec(lra_ctx* ctx, const void* D, void* out, int64_t batch, int64_t n_frames, int n_bins, const double* t_out_host, int64_t n_out, int dtype);

/* ---- PCEN: librosa.pcen, librosa/core/spectrum.py:2396-2666 (the consumer of the streaming STFT in
 * docs/examples/plot_pcen_stream.py:71-80) ---------------------------------------------------------------------------------- */
/* S, ref: [rows][n_frames] real of `dtype` (device), time on the last axis; ref = the array the smoother runs over (NULL: S itself,
 * i.e. max_size == 1 and no ref=, :2628-2630).  out: [rows][n_frames] FLOAT64 whatever `dtype` is -- the reference's filter state
 * is float64 and promotes everything after it (:2649-2665).
 *   M = scipy.signal.lfilter([b], [1, b - 1], ref, zi, axis=time)   smooth = exp(-gain (log eps + log1p(M / eps)))
 *   out = log1p(S smooth) | exp(power (log S + log smooth)) | bias**power expm1(power log1p(S smooth / bias))   (power == 0 | bias == 0 | else)
 * zi: device float64 [rows] initial filter state (a previous call's zf) or NULL = zi_scalar for every row (the caller's
 * scipy.signal.lfilter_zi([b], [1, b - 1]), :2649-2652).  zf: device float64 [rows] final state or NULL (return_zf, :2655). */
int lra_pcen_exec(lra_ctx* ctx, const void* S, const void* ref, void* out, int64_t rows, int64_t n_frames, int dtype, double b, double gain, double bias, double power, double eps,
                  const void* zi, double zi_scalar, void* zf);

/* scipy.ndimage.maximum_filter1d(S, size, axis) with mode="reflect", origin 0 -- pcen's max_size > 1 (:2640-2642).  S, out:
 * [outer][n_bands][inner] of `dtype` (device), the filter runs over n_bands: out[m] = max(S[m - size/2 .. m - size/2 + size - 1]). */
int lra_maxfilter_exec(lra_ctx* ctx, const void* S, void* out, int64_t outer, int n_bands, int64_t inner, int size, int dtype);

/* ---- onset strength: librosa.onset.onset_strength / onset_strength_multi, librosa/onset.py:217-367, 445-645 ----------------------- */
#define LRA_ONSET_NONE 0    /* aggregate=False (not callable): one row per band (:619-622) */
#define LRA_ONSET_MEAN 1    /* np.mean over each channel's bands (util.sync, util/utils.py:1785-1814; :612-622) */
#define LRA_ONSET_SUM 2
#define LRA_ONSET_MAX 3
#define LRA_ONSET_MIN 4
#define LRA_ONSET_MEDIAN 5  /* exact np.median: the mean of the two middle values for an even count */
#define LRA_ONSET_ROWS 6    /* S already holds the aggregated rows (a host-side aggregate callable): pad, trim and detrend only */
/* S: [batch][n_bands][n_frames] of `dtype` (device), the mel kernel's layout.  fuse_db != 0: S is a power spectrogram and the flux is
 * taken of power_to_db(|S|, ref=1, amin, top_db) (:579-583), evaluated while S is read; item_max (device, [batch]) is the per-item max
 * of |S| (lra_item_max_exec).  Otherwise S is used as given (:585-589).  ref: the caller's reference of S's shape, used as given (:601-604),
 * or NULL: S itself (max_size == 1) or maximum_filter1d(S, max_size, axis=bands, mode="reflect") (:594-600).
 *   env[b][m][t] = max(0, S[b][m][t + lag] - ref[b][m][t]),  0 <= t < n_frames - lag (:606-610)
 * Aggregates run over channels: channel c holds the bands ch_bands[ch_offsets[c] .. ch_offsets[c + 1]) (device int32 arrays;
 * max_ch_bands = the largest channel's band count), or both NULL: one channel of every band in order (channels=None; n_ch = 1,
 * max_ch_bands = n_bands); NONE / ROWS write one row per band and ignore them.
 * out: [batch][rows][n_out], rows = n_ch (aggregates) or n_bands; out[.][.][j] = agg(env)[j - pad] where that index lies in the
 * envelope, 0 elsewhere (the left padding and the trim of :624-642).  detrend != 0: out is FLOAT64, scipy.signal.lfilter([1, -1],
 * [1, -0.99], ., axis=-1) of those rows from a zero state (:635-638); env (device) is scratch of batch * rows * n_out elements of
 * `dtype`.  Empty channels: NaN for mean / median, 0 for sum; max / min reject them (np.max raises). */
int lra_onset_exec(lra_ctx* ctx, const void* S, const void* ref, void* out, int64_t batch, int n_bands, int64_t n_frames, int dtype, int lag, int max_size, int aggregate,
                   const int32_t* ch_offsets, const int32_t* ch_bands, int n_ch, int max_ch_bands, int64_t pad, int64_t n_out, int fuse_db, double amin, double top_db,
                   const void* item_max, int detrend, void* env);

/* ---- tempogram and tempo: librosa.feature.tempogram / tempo, librosa/feature/rhythm.py:38-191, 295-471 ------------------------------ */
#define LRA_TEMPOGRAM_WRITE 0   /* the normalised tempogram, out: float64 [batch][win_length][n_frames] (:173-191) */
#define LRA_TEMPOGRAM_SUM 1     /* tempo(aggregate=np.mean), out: float64 [batch] BPM (:445-471) */
#define LRA_TEMPOGRAM_ARGMAX 2  /* tempo(aggregate=None), out: float64 [batch][n_frames] BPM per frame */
#define LRA_TEMPOGRAM_NORM_NONE 0
#define LRA_TEMPOGRAM_NORM_INF 1
#define LRA_TEMPOGRAM_NORM_L1 2
#define LRA_TEMPOGRAM_NORM_L2 3
/* Bytes of device scratch `work` that lra_tempogram_exec needs for these sizes (n_frames: the tempogram's frame count). */
int64_t lra_tempogram_work_bytes(int64_t batch, int64_t n_frames, int win_length, int mode);
/* env: [batch][n] onset envelopes of `dtype` (device).  center != 0: np.pad(env, win_length // 2, mode="linear_ramp", end_values=0) and
 * the first n frames (:167-182), else n - win_length + 1 frames (n >= win_length).  Each frame of hop 1 times window (device float64
 * [win_length], get_window(window, win_length, fftbins=True)) is autocorrelated in float64 up to lag win_length - 1 (core/audio.py:1320-1394)
 * and normalised per column by util.normalize(norm, axis=-2) with threshold tiny and fill=None (util/utils.py:797-1020).
 * SUM / ARGMAX then score log1p(1e6 tg) + logprior (device float64 [win_length]) and take np.argmax's index (the first NaN, else the first
 * maximum) into bpms (device float64 [win_length]): SUM on the mean over frames (group sums added in a fixed order, then / n_frames),
 * ARGMAX per frame.  work: device scratch of lra_tempogram_work_bytes bytes.  nonfinite (host, may be NULL): set to 1 when some column of
 * the autocorrelation is not finite (normalize raises for every norm, :865-866) -- reading it waits for the stream. */
int lra_tempogram_exec(lra_ctx* ctx, const void* env, int64_t batch, int64_t n, int dtype, int win_length, int center, const void* window, int norm, int mode,
                       const void* logprior, const void* bpms, void* out, void* work, int* nonfinite);

/* ---- beat tracking: librosa.beat.beat_track's dynamic program, librosa/beat.py:510-741 ---------------------------------------------- */
#define LRA_BEAT_BPM_PER_ROW 0    /* bpm: float64 [batch], one tempo per envelope (:298-301) */
#define LRA_BEAT_BPM_PER_FRAME 1  /* bpm: float64 [batch][n], a tempo per frame (:598-608, :639) */
/* Bytes of device scratch `work` that lra_beat_exec needs for these sizes. */
int64_t lra_beat_work_bytes(int64_t batch, int64_t n, int bpm_mode);
/* env: [batch][n] onset envelopes of `dtype` (device); bpm: device float64 (see the modes), every value > 0 (:533).  Per row:
 * x / (std(ddof=1) + tiny) in `dtype` (:567-570), frames_per_beat = round(frame_rate * 60 / bpm) half-even in float64 (:546), the local
 * score (:576-608; one rounding to `dtype` per term, increasing k), the recurrence in float64 with tightness rounded to float32 (:619-660;
 * the largest predecessor wins a tie), the last beat (:697-729), the walk along the back-links (:736-741) and the trim with threshold
 * 0.5 rms of the Hann-smoothed beat scores, or 0 with trim == 0 (:667-694).  out: uint8 [batch][n], 1 = beat.  Rows the reference cannot
 * handle get no beats: n < 2, a row without a non-zero entry, frames_per_beat outside [2, 2^29].  work: device scratch of
 * lra_beat_work_bytes bytes.  any_nonzero (host, may be NULL): set to 1 when some entry of env is non-zero (:280) -- reading it waits for
 * the stream. */
int lra_beat_exec(lra_ctx* ctx, const void* env, int64_t batch, int64_t n, int dtype, const void* bpm, int bpm_mode, double frame_rate, double tightness, int trim, void* out,
                  void* work, int* any_nonzero);

/* ---- peak picking and onset backtracking: librosa.util.peak_pick (util/utils.py:1183-1496), onset_detect's normalisation (onset.py:164-176),
 * onset_backtrack's preceding minimum (onset.py:430-441) -------------------------------------------------------------------------------- */
#define LRA_PEAK_GREEDY 0    /* the earliest frame first (:1188-1217) */
#define LRA_PEAK_DP_COUNT 1  /* the most peaks (:1225-1281, count) */
#define LRA_PEAK_DP_VALUE 2  /* the largest sum of peak values */
#define LRA_PEAK_ANY_NONZERO 1  /* status bit 0: some entry is non-zero */
#define LRA_PEAK_ALL_FINITE 2   /* status bit 1: every entry is finite */
/* Bytes of device scratch `work` that lra_peak_pick_exec needs for these sizes. */
int64_t lra_peak_pick_work_bytes(int64_t batch, int64_t n, int method);
/* x: [batch][n] rows of `dtype` (device).  normalize != 0: per row x - min, then / (max of that + tiny), each one rounding in `dtype` (the
 * bits NumPy gives).  A frame is a candidate when x[i] == max(x[i - pre_max : i + post_max]) (a NaN in the window: never for GREEDY, always
 * for the DP methods, as the reference's comparisons) and x[i] >= mean(x[i - pre_avg : i + post_avg]) + delta, the mean and the comparison in
 * float64 (the reference's mean is rounded to `dtype`: the two agree wherever the difference is not within that rounding).  GREEDY: the
 * earliest candidate, then the earliest more than `wait` frames later, and so on.  DP_*: the reference's backward recurrence in float64 and
 * the walk along its pointers.  Windows and `wait` beyond n count as n.  out: uint8 [batch][n], 1 = peak.  norm_out (may be NULL): receives
 * the normalised rows (a copy of x with normalize == 0).  work: device scratch of lra_peak_pick_work_bytes bytes.  status (host, may be
 * NULL): LRA_PEAK_ANY_NONZERO | LRA_PEAK_ALL_FINITE over all normalised rows (onset.py:176) -- reading it waits for the stream. */
int lra_peak_pick_exec(lra_ctx* ctx, const void* x, int64_t batch, int64_t n, int dtype, int normalize, int64_t pre_max, int64_t post_max, int64_t pre_avg, int64_t post_avg,
                       double delta, int64_t wait, int method, void* out, void* norm_out, void* work, int* status);
/* energy: [batch][m] rows of `dtype` (device).  out: int32 [batch][m], out[i] = the largest j <= i with j == 0, or with 1 <= j <= m - 2,
 * e[j] <= e[j - 1] and e[j] < e[j + 1]: onset_backtrack(events, energy) is out[min(events, m - 1)]. */
int lra_prev_minimum_exec(lra_ctx* ctx, const void* energy, int64_t batch, int64_t m, int dtype, void* out);

/* ---- chroma: librosa.feature.chroma_stft / chroma_cqt (feature/spectral.py:1285-1293, 1407-1421) ------------------------------------
 * raw[c][t] = sum_f W[c][f] X[f][t]; has_threshold != 0: raw < threshold -> 0 (chroma_cqt); then util.normalize(raw, norm, axis=-2) with
 * fill=None (util/utils.py:959-1011): the frame's length from float64 magnitudes, 1 where it is below `tiny` of `dtype`, one division. */
#define LRA_CHROMA_NORM_NONE 0
#define LRA_CHROMA_NORM_L1 1
#define LRA_CHROMA_NORM_L2 2
#define LRA_CHROMA_NORM_INF 3
/* X: `dtype` (device), element (b, f, t) at b * batch_stride + f * bin_stride + t * frame_stride (elements).  bin_stride == 1 (the layout
 * lra_spectrogram_exec writes, rows possibly padded) and frame_stride == 1 (a C-contiguous [b][f][t] array) are the two fast forms; any
 * other strides are served by the second.  W: [n_chroma][n_bins] `dtype` (device).  out: [batch][n_chroma][n_frames] `dtype`.  work: at
 * least 256 bytes of device scratch.  nonfinite (host, may be NULL): 1 when some raw value, after the threshold, is NaN or infinite (the
 * reference then raises "Input must be finite", for every norm) -- reading it waits for the stream. */
int lra_chroma_exec(lra_ctx* ctx, const void* X, int64_t batch, int64_t n_bins, int64_t n_frames, int64_t batch_stride, int64_t bin_stride, int64_t frame_stride, int dtype,
                    const void* W, int64_t n_chroma, int norm, double threshold, int has_threshold, void* out, void* work, int* nonfinite);

/* ---- pitch tracking and tuning: librosa.piptrack, pitch_tuning, estimate_tuning (core/pitch.py:28-366) -----------------------------------
 * S: magnitudes of `dtype` (device), element (b, f, t) at b * batch_stride + f * bin_stride + t * frame_stride (elements); |.| is taken on
 * load.  bin_stride == 1 (the layout lra_spectrogram_exec writes, rows possibly padded) and frame_stride == 1 (a C-contiguous [b][f][t]
 * array) are the two fast forms; any other strides are served by the second.  Bins bin_lo <= f < bin_hi pass the frequency mask.  A bin is
 * a peak where x = S * (S > ref_value) has x[f] > x[f - 1] and x[f] >= x[f + 1] (bin 0 never, the last bin on the first test alone); there
 * pitches = (f + shift) * sr / n_fft (float64, rounded once) and mags = S + 0.5 * gradient * shift with shift = -b / a of the parabola
 * through the three bins (0 where |b| >= |a| and at the last bin); every other element is 0. */
#define LRA_PITCH_REF_MAX 0     /* ref_value = (dtype)threshold * max over ALL bins of the frame */
#define LRA_PITCH_REF_ROW 1     /* ref_value = ref_row[b * n_frames + t]: float64 (device), the threshold already applied */
#define LRA_PITCH_REF_SCALAR 2  /* ref_value = ref_scalar */
/* pitches, mags: `dtype` (device), element (b, f, t) at b * out_batch_stride + f * out_bin_stride + t * out_frame_stride; every element
 * with f < n_bins is written. */
int lra_piptrack_exec(lra_ctx* ctx, const void* S, int64_t batch, int64_t n_bins, int64_t n_frames, int64_t batch_stride, int64_t bin_stride, int64_t frame_stride, int dtype,
                      int64_t bin_lo, int64_t bin_hi, int ref_mode, double threshold, const void* ref_row, double ref_scalar, double sr, int64_t n_fft, void* pitches, void* mags,
                      int64_t out_batch_stride, int64_t out_bin_stride, int64_t out_frame_stride);
/* Bytes of device scratch `work` that lra_tuning_exec needs: every frame owns ceil(masked_bins / 2) peak slots (two adjacent bins are never
 * both peaks), masked_bins = bin_hi - bin_lo. */
int64_t lra_tuning_work_bytes(int64_t batch, int64_t n_frames, int64_t masked_bins, int dtype);
/* estimate_tuning without the dense arrays: the tracker emits its peaks with pitch > 0, a radix select finds thr = np.median of their
 * magnitudes (the mean of the two middle values in `dtype`; 0 without peaks), and the peaks with mag >= thr enter the histogram of
 * lra_pitch_tuning_exec.  out: int64 [n_hist + 2] (device): the counts, the number of peaks that entered, the number of peaks.  Integer
 * atomics only: the same bits on every run.  Nothing is read back here. */
int lra_tuning_exec(lra_ctx* ctx, const void* S, int64_t batch, int64_t n_bins, int64_t n_frames, int64_t batch_stride, int64_t bin_stride, int64_t frame_stride, int dtype,
                    int64_t bin_lo, int64_t bin_hi, int ref_mode, double threshold, const void* ref_row, double ref_scalar, double sr, int64_t n_fft, const void* edges, int64_t n_hist,
                    double bins_per_octave, void* work, void* out);
/* pitch_tuning's histogram: of the n frequencies freq (`dtype`, device) those > 0 give residual = mod(bins_per_octave * log2(f / 27.5), 1),
 * minus 1 where >= 0.5, in `dtype`; np.histogram(residual, edges) with edges float64 [n_hist + 1] (device), the last bin closed.
 * out: int64 [n_hist + 2] (device): the counts, the number of frequencies > 0, 0. */
int lra_pitch_tuning_exec(lra_ctx* ctx, const void* freq, int64_t n, int dtype, const void* edges, int64_t n_hist, double bins_per_octave, void* out);

/* ---- yin and the front half of pyin: librosa.yin, librosa/core/pitch.py:369-628 ------------------------------------------------------- */
#define LRA_YIN_F0 0      /* f0: float64 [batch][n_frames]; nothing dense is written */
#define LRA_YIN_FRAMES 1  /* frames, shifts: `dtype` [batch][max_period - min_period + 1][n_frames]: the CMND and the parabolic shifts */
/* y: [batch][n] samples of `dtype` (device), never written.  center != 0: np.pad(y, frame_length // 2, mode=pad_mode) folded into the load
 * (pad_mode: 0 constant, 1 reflect, 2 edge, 3 symmetric); n_frames = 1 + (n + 2 pad - frame_length) / hop_length.  Per frame, in float64:
 * d(k) = 2 (acf(0) - acf(k)) - E(k - 1) for k = 1 .. max_period with E = cumsum(y^2) and E(0) read as 0 (:394-406), the cumulative mean
 * normalised difference c = d(k) / (mean(d(1 .. k)) + tiny) for min_period <= k <= max_period (:408-418) and the parabolic shifts
 * (:421-477).  F0: the first trough of c below trough_threshold (util.localmin, with c[0] < c[1] at the first lag), else np.argmin(c);
 * f0 = sr / (min_period + index + shift) (:595-628).  1 <= min_period < max_period <= frame_length - 1.  The autocorrelation goes through the
 * smallest mixed-radix transform of at least frame_length + max_period points, or a direct sum where there is none.  The direct sum keeps
 * 16 max_period bytes in LDS: lra_yin_lds_bytes above LRA_YIN_LDS_MAX is refused (LRA_EINVAL).  Pointers of the other mode may be NULL. */
/* Bytes of LDS a workgroup of lra_yin_exec needs for these sizes (host arithmetic only, no device is touched); the call is served when this
 * is at most LRA_YIN_LDS_MAX.  Only a direct-kernel call (frame_length + max_period above the largest compiled transform, 4800) with
 * max_period > 10239 exceeds it. */
#define LRA_YIN_LDS_MAX (160 * 1024)
int64_t lra_yin_lds_bytes(int frame_length, int max_period);
int lra_yin_exec(lra_ctx* ctx, const void* y, int64_t batch, int64_t n, int dtype, int frame_length, int hop_length, int center, int pad_mode, int min_period, int max_period,
                 double trough_threshold, double sr, int mode, void* f0, void* frames, void* shifts);

/* ---- sequence.viterbi, viterbi_discriminative, viterbi_binary: librosa/sequence.py:1174-1259 (_viterbi), 1280-1432, 1455-1679, 1702-1874 --- */
#define LRA_VITERBI_GENERATIVE 0      /* log_prob = log(prob + eps)                                   (:1395) */
#define LRA_VITERBI_DISCRIMINATIVE 1  /* log_prob = log(prob + eps) - log_marginal[state]             (:1653) */
#define LRA_VITERBI_BINARY 2          /* prob [chain][step]; the rows 1 - p and p of a 2-state chain, minus log_marginal[chain % n_labels][row] (:1853-1854) */
#define LRA_VITERBI_LOG 3             /* prob is a float64 log table already: the transpose alone */
#define LRA_VITERBI_FLAG_NEGATIVE 1   /* some prob < 0 */
#define LRA_VITERBI_FLAG_ABOVE_ONE 2  /* some prob > 1 */
#define LRA_VITERBI_FLAG_COLUMN_SUM 4 /* DISCRIMINATIVE: some column's sum over the states is not np.allclose to 1 */
#define LRA_VITERBI_LDS_MAX (160 * 1024)
#define LRA_VITERBI_MAX_STATES 8192
/* Bytes of LDS a decode workgroup needs for n_states and the longest predecessor list n_pred (0: full search); host arithmetic only.  Two
 * float64 value rows (16 n_states bytes) and the argmax scratch, plus log_trans where a full search's table fits beside them; up to
 * LRA_VITERBI_SMALL_MAX states, a table per chain of the workgroup.  Above LRA_VITERBI_MAX_STATES the answer exceeds LRA_VITERBI_LDS_MAX
 * and lra_viterbi_exec refuses (LRA_EINVAL). */
int64_t lra_viterbi_lds_bytes(int n_states, int n_pred);
/* prob: [chains][n_states][n_steps] of `dtype` (device; BINARY: [chains][n_steps], n_states = 2), never written -> log_prob: float64
 * [chains][n_steps][n_states].  The logarithm is taken in `dtype` after adding eps (util.tiny of prob's type) and widened exactly; BINARY takes
 * 1 - p in `dtype` and both logarithms in float64.  log_marginal: float64 [n_states] (DISCRIMINATIVE) or [n_labels][2] (BINARY), else NULL.
 * work: 4 bytes (device).  *flags: the LRA_VITERBI_FLAG_* bits met (this waits for the stream); the caller raises before it decodes. */
int lra_viterbi_prep_exec(lra_ctx* ctx, const void* prob, int dtype, int kind, int64_t chains, int n_states, int64_t n_steps, double eps, const void* log_marginal, int n_labels,
                          void* log_prob, void* work, int* flags);
/* _viterbi (:1174-1259) of every chain: value[0] = log_prob[0] + log_p_init; value[t][j] = log_prob[t][j] + max_k (value[t - 1][k] + log_trans[k][j]),
 * the first k on a tie and 0 where every candidate is -inf; the last state np.argmax(value[-1]); the pointers walked back.  Chain c reads table
 * c % n_tables of log_trans [n_tables][n_states][n_states] and log_p_init [n_tables][n_states] (float64, device); n_tables > 1 only up to
 * LRA_VITERBI_SMALL_MAX states.  threshold: -inf for the full search; otherwise only k with log_trans[k][j] >= threshold are candidates, and above
 * LRA_VITERBI_SMALL_MAX states they come as lists, ascending in k: pred_k uint16 [n_pred][n_states], pred_lt float64 [n_pred][n_states], pred_n int32
 * [n_states] (device).  ptr: uint16 scratch [chains][n_steps][n_states].  states: uint16 [chains][n_steps]; logp: float64 [chains]. */
#define LRA_VITERBI_SMALL_MAX 32
int lra_viterbi_exec(lra_ctx* ctx, const void* log_prob, int64_t chains, int n_states, int64_t n_steps, const void* log_trans, const void* log_p_init, int n_tables, double threshold,
                     int n_pred, const void* pred_k, const void* pred_lt, const void* pred_n, void* ptr, void* states, void* logp);

/* ---- sequence.dtw and dtw_backtracking: librosa/sequence.py:185-694 ----------------------------------------------------------------------- */
#define LRA_DTW_MAX_STEPS 16 /* rows of a step table, the three defaults (1, 1), (0, 1), (1, 0) included */
#define LRA_DTW_MAX_STEP 8   /* the largest step component */
#define LRA_DTW_EUCLIDEAN 0
#define LRA_DTW_SQEUCLIDEAN 1
#define LRA_DTW_CITYBLOCK 2
#define LRA_DTW_COSINE 3
#define LRA_DTW_I32 2 /* types of a given C besides LRA_F32 and LRA_F64 */
#define LRA_DTW_I64 3
#define LRA_DTW_U8 4
#define LRA_DTW_FLAG_NAN 1         /* C holds a NaN */
#define LRA_DTW_FLAG_END_INF 2     /* D[-1, -1] is infinite (no subseq) */
#define LRA_DTW_FLAG_ROW_INF 4     /* every entry of D[-1] is infinite (subseq) */
#define LRA_DTW_FLAG_NOT_ORIGIN 8  /* the path does not end at (0, 0) (no subseq) */
#define LRA_DTW_FLAG_BAD_STEP 16   /* the step matrix holds an index outside the step table */
#define LRA_DTW_START_END (-1)     /* backtrack from (N - 1, M - 1) */
#define LRA_DTW_START_ARGMIN (-2)  /* backtrack from (N - 1, np.argmin(D[-1])) */
/* Bytes of LDS a tile of lra_dtw_accumulate_exec needs (host arithmetic only): D with its halo, C and the step indices of a tile of edge `tile`
 * (0: the library's choice).  0 for arguments the accumulation refuses. */
int64_t lra_dtw_lds_bytes(int tile, int max_0, int max_1);
/* C[n][m] = metric(X[:, n], Y[:, m]) in float64 (device, [N][M]) from X [n_features][N] and Y [n_features][M] of `dtype` (device, never
 * written), the features summed in ascending order; a zero vector under LRA_DTW_COSINE gives NaN.  work: 16 bytes (device).  *flags:
 * LRA_DTW_FLAG_NAN where C holds one (this waits for the stream). */
int lra_dtw_cost_exec(lra_ctx* ctx, const void* X, const void* Y, int dtype, int64_t n_features, int64_t N, int64_t M, int metric, void* C, void* work, int* flags);
/* A given C of `dtype` (LRA_F32, LRA_F64, LRA_DTW_I32, LRA_DTW_I64, LRA_DTW_U8; `count` elements, device, never written) -> float64 in `out`,
 * and the NaN flag as above.  out may be NULL for LRA_F64: the check alone. */
int lra_dtw_prepare_exec(lra_ctx* ctx, const void* C, int dtype, int64_t count, void* out, void* work, int* flags);
/* __dtw_calc_accu_cost (:502-571) of C float64 [N][M] (device): D float64 [N][M] and the index of the step that reached each cell, uint8 [N][M]
 * (0 where none improved it).  steps: int32 [n_steps][2], weights_add, weights_mul: float64 [n_steps] (HOST arrays).  D starts at +inf, at
 * C[0][0] in (0, 0) and, with subseq, at C[0][:] in the first row.  band: C reads as +inf where m - n >= band_hi or m - n <= band_lo.  tile: 0
 * for the library's choice, or 8, 16, 32 or 64; the result does not depend on it.  One launch per tile anti-diagonal, in stream order. */
int lra_dtw_accumulate_exec(lra_ctx* ctx, const void* C, int64_t N, int64_t M, const int32_t* steps, const double* weights_add, const double* weights_mul, int n_steps, int subseq, int band,
                            int64_t band_lo, int64_t band_hi, int tile, void* D, void* step_idx);
/* uint8 step indices -> int32, `count` elements (device). */
int lra_dtw_widen_exec(lra_ctx* ctx, const void* step_idx, int64_t count, void* out);
/* __dtw_backtracking (:575-640) over step_idx [N][M] (uint8, or int32 with steps_i32; device) and the step table steps int32 [n_steps][2]
 * (HOST): from column `start` of the last row (or LRA_DTW_START_*), until row 0 (subseq) or (0, 0), or until an index goes negative.  D: float64
 * [N][M] or NULL; with it the LRA_DTW_FLAG_END_INF / ROW_INF checks are made first and a flagged call writes no path.  path: int64
 * [N + M - 1][2] (device); work: 16 bytes (device).  *length: pairs written; *status: the flags met (this waits for the stream). */
int lra_dtw_backtrack_exec(lra_ctx* ctx, const void* D, const void* step_idx, int steps_i32, int64_t N, int64_t M, const int32_t* steps, int n_steps, int subseq, int64_t start, void* path,
                           void* work, int64_t* length, int* status);

/* ---- sequence.rqa: librosa/sequence.py:698-1074 --------------------------------------------------------------------------------------------- */
#define LRA_RQA_WORK_BYTES (16 + 16 * 1024) /* the work area of lra_rqa_argmax_exec and lra_rqa_backtrack_exec (device) */
/* Bytes of LDS a workgroup of lra_rqa_score_exec needs (host arithmetic only) for blocks of `rows` rows and strips of `strip` columns (0: the
 * library's choice): three rows of strip + 2 (rows - 1) + 2 pairs of float64.  0 for a geometry that is not served: rows is a
 * power of two up to 64, strip a power of two from 4 to 1024. */
int64_t lra_rqa_lds_bytes(int rows, int strip);
/* __rqa_dp (:869-1023) of sim [N][M] of `dtype` (LRA_F32 or LRA_F64; device, never written): score [N][M] of the same type and the pointers int8
 * [N][M] (device): 0 diagonal, 1 the left knight (-1, -2), 2 the up knight (-2, -1), -1 a reset outside the path, -2 the start of a sequence.
 * Candidates are formed in float64, each operation rounded on its own, and the score is rounded once to `dtype` by the store; np.argmax's order
 * (the first maximum, a NaN first).  One launch per block of `rows` rows, in stream order; the result does not depend on (rows, strip). */
int lra_rqa_score_exec(lra_ctx* ctx, const void* sim, int dtype, int64_t N, int64_t M, double gap_onset, double gap_extend, int knight_moves, int rows, int strip, void* score,
                       void* pointers);
/* np.argmax(score) over `count` elements of `dtype` (device): the flat index goes to the first 8 bytes of work (LRA_RQA_WORK_BYTES, device). */
int lra_rqa_argmax_exec(lra_ctx* ctx, const void* score, int dtype, int64_t count, void* work);
/* __rqa_backtrack (:1026-1074) over the pointers of lra_rqa_score_exec from the cell lra_rqa_argmax_exec left in work: the path in ascending
 * order in the LAST *length rows of path, uint64 [min(N, M)][2] (device) (this waits for the stream). */
int lra_rqa_backtrack_exec(lra_ctx* ctx, const void* pointers, int64_t N, int64_t M, void* work, void* path, int64_t* length);

/* ---- segment.cross_similarity and recurrence_matrix: librosa/segment.py:67-357, :361-706, __affinity_bandwidth :1332-1437 ------------------- */
#define LRA_KNN_MAX_K 2048     /* the longest neighbour list a query frame keeps */
#define LRA_KNN_WORK_BYTES 64  /* the work area of the calls below (device) */
#define LRA_KNN_CONNECTIVITY 0
#define LRA_KNN_DISTANCE 1
#define LRA_KNN_AFFINITY 2
#define LRA_KNN_BW_SCALAR 0 /* a given scalar, or np.nanmedian of the rows' distance to the bandwidth_k-th neighbour left in the work area */
#define LRA_KNN_BW_MEAN_K 1
#define LRA_KNN_BW_GMEAN_K 2
#define LRA_KNN_BW_MEAN_K_AVG 3
#define LRA_KNN_BW_GMEAN_K_AVG 4
#define LRA_KNN_BW_MEAN_K_AVG_AND_PAIR 5
#define LRA_KNN_BW_MATRIX 6 /* a float64 matrix [n][m], gathered at the stored entries */
#define LRA_KNN_STATUS_EMPTY_GRAPH 1  /* no row has a finite distance to its bandwidth_k-th neighbour */
#define LRA_KNN_STATUS_ROW_EMPTY 2    /* a row stores no entry */
#define LRA_KNN_STATUS_NON_POSITIVE 4 /* an entry of the bandwidth matrix is <= 0 */
/* Bytes of LDS a workgroup of lra_knn_select_exec needs (host arithmetic only) for `rows` query frames per workgroup, candidate tiles of
 * `tile` frames (0: the library's choice) and lists of k pairs.  0 for a geometry that is not served: rows is a power of two up to 16, tile a
 * power of two from 4 to 1024, rows * tile <= 2048, k <= LRA_KNN_MAX_K, and everything fits 64 KiB. */
int64_t lra_knn_lds_bytes(int rows, int tile, int k);
/* The k nearest candidates of every query frame: Q [n_features][n] and R [n_features][m] of `dtype` (LRA_F32 or LRA_F64; device, never written),
 * `metric` one of LRA_DTW_EUCLIDEAN ... LRA_DTW_COSINE, summed over the features in ascending order in float64, every operation rounded on its own.  The candidates of frame i are the j with
 * |i - j| >= width (width 0: all) and, with skip_zero, a distance that is not exactly 0; pairs are ordered by distance, ties by the lower index, a
 * NaN last.  count int32 [n], index int32 [n][k] ascending in each row, distance float64 [n][k] (device).  No buffer of n * m elements is used;
 * the result does not depend on (rows, tile). */
int lra_knn_select_exec(lra_ctx* ctx, const void* Q, const void* R, int dtype, int64_t n_features, int64_t n, int64_t m, int metric, int k, int64_t width, int skip_zero, int rows, int tile,
                        void* count, void* index, void* distance);
/* keep uint8 [n][k] (device): an entry stays unless drop_zero and its distance is exactly 0, or sym and frame i is not in the list of frame j. */
int lra_knn_mutual_exec(lra_ctx* ctx, int64_t n, int k, const void* count, const void* index, const void* distance, int sym, int drop_zero, void* keep);
/* Per row, over the kept distances (keep null: all) and, with add_self, a 0 for the self link: dist_to_k, the min(bandwidth_k, stored)-th smallest,
 * and avg, the mean of those first ones (float64 [n], device; NaN for an empty row).  With `median`, np.nanmedian(dist_to_k) is left in the work
 * area for LRA_KNN_BW_SCALAR.  *status: LRA_KNN_STATUS_* bits; *first_empty: the lowest empty row (this waits for the stream). */
int lra_knn_bandwidth_exec(lra_ctx* ctx, int64_t n, int k, const void* count, const void* distance, const void* keep, int add_self, int bandwidth_k, int median, void* dist_to_k, void* avg,
                           void* work, int* status, int64_t* first_empty);
/* (matrix <= 0).any() of a float64 bandwidth matrix (device) -> LRA_KNN_STATUS_NON_POSITIVE in *status (this waits for the stream). */
int lra_knn_bw_check_exec(lra_ctx* ctx, const void* matrix, int64_t count, void* work, int* status);
/* The result of the lists: entry (i, j) holds 1 (uint8, LRA_KNN_CONNECTIVITY), the distance, or exp(distance / -bandwidth) (float64), and with
 * `self` the link (i, i) at distance 0 is stored too.  Either the transposed dense result `dense` [m][n] (zero elsewhere), or, dense null, the
 * compressed arrays: indptr int32 [n + 1], indices int32 and data [*total] in ascending order per row, counts int32 [n] scratch (device;
 * this waits for the stream).  bw_on_device: LRA_KNN_BW_SCALAR reads lra_knn_bandwidth_exec's median from the work area instead of bw_scalar;
 * sigma: dist_to_k or avg, as bw_mode asks; matrix: LRA_KNN_BW_MATRIX's. */
int lra_knn_emit_exec(lra_ctx* ctx, int64_t n, int64_t m, int k, const void* count, const void* index, const void* distance, const void* keep, int self, int mode, int bw_mode,
                      double bw_scalar, int bw_on_device, const void* sigma, const void* matrix, void* work, void* counts, void* indptr, void* indices, void* data, void* dense,
                      int64_t* total);
/* The same result where every candidate is kept, straight from the distances: out [m][n] (device) with out[j][i] the value of entry (i, j) for
 * |i - j| >= width (and, but for connectivity, a distance that is not exactly 0), the self link as above, 0 elsewhere. */
int lra_knn_dense_exec(lra_ctx* ctx, const void* Q, const void* R, int dtype, int64_t n_features, int64_t n, int64_t m, int metric, int64_t width, int self, int mode, int bw_mode,
                       double bw_scalar, int bw_on_device, const void* sigma, const void* matrix, void* work, void* out);

/* ---- segment.path_enhance, util.shear / recurrence_to_lag / lag_to_recurrence, feature.stack_memory: librosa/segment.py:1167-1329, :709-891,
 * librosa/util/utils.py:2136-2260, librosa/feature/utils.py:134-314 ------------------------------------------------------------------------- */
#define LRA_ENHANCE_LDS_MAX (160 * 1024)
#define LRA_ENHANCE_MAX_REACH 124 /* rows, and columns, the filters of one call may span beyond one cell: that halo fits the LDS next to the smallest tile */
#define LRA_ENHANCE_REFLECT 0     /* scipy.ndimage's boundary modes */
#define LRA_ENHANCE_CONSTANT 1
#define LRA_ENHANCE_NEAREST 2
#define LRA_ENHANCE_MIRROR 3
#define LRA_ENHANCE_WRAP 4
#define LRA_STACK_CONSTANT 0 /* np.pad's modes */
#define LRA_STACK_EDGE 1
#define LRA_STACK_REFLECT 2
#define LRA_STACK_SYMMETRIC 3
#define LRA_STACK_WRAP 4
/* One non-zero weight of a filter: out[i][j] += R[ext(i + dr)][ext(j + dc)] * w. */
typedef struct lra_enhance_tap {
    int32_t dr, dc;
    double w;
} lra_enhance_tap;
/* Bytes of the device table lra_path_enhance_exec writes for n_taps taps in n_filters filters. */
#define LRA_ENHANCE_TABLE_BYTES(n_taps, n_filters) ((((size_t)(n_filters) + 1) * 4 + 15) / 16 * 16 + 16 * (size_t)(n_taps))
/* Bytes of LDS a workgroup of lra_path_enhance_exec needs (host arithmetic only) for an output tile of rows x cols cells under a halo of
 * halo_rows rows and halo_cols columns; rows == cols == 0: the library's choice.  0 for a geometry that is not served: rows 1 .. 256, cols
 * 16, 32 or 64, rows * cols <= 4096, and tile plus halo as float64 within LRA_ENHANCE_LDS_MAX. */
int64_t lra_enhance_lds_bytes(int rows, int cols, int halo_rows, int halo_cols);
/* np.maximum over the n_filters responses scipy.ndimage.convolve gives, then np.clip(., 0, None) with `clip`: R and out [channels][h][w] of
 * `dtype` (LRA_F32 or LRA_F64; device, R never written).  taps (host): the non-zero weights of filter f at starts[f] .. starts[f + 1] - 1
 * (starts: host, n_filters + 1 entries from 0), summed in that order in float64 from 0, every product and sum rounded on its own; a float32
 * response is rounded once.  ext: `mode` (LRA_ENHANCE_*), LRA_ENHANCE_CONSTANT reads cval outside.  All taps lie within a box of at most
 * LRA_ENHANCE_MAX_REACH rows and columns around the cell.  table: LRA_ENHANCE_TABLE_BYTES of device scratch (this waits for the stream while it
 * is filled).  (rows, cols): the tile, 0, 0 for the library's choice; the result does not depend on it. */
int lra_path_enhance_exec(lra_ctx* ctx, const void* R, int dtype, int64_t channels, int64_t h, int64_t w, const lra_enhance_tap* taps, const int32_t* starts, int n_filters, int mode,
                          double cval, int clip, int rows, int cols, void* table, void* out);
/* util.shear with the zero padding and the slice of the lag transforms folded in: `in` [rows_in][cols_in] and out [rows_out][cols_out] of
 * esize-byte elements (1, 2, 4 or 8; device).  axis 1: out[r][c] = P[(r - factor c) mod period][c]; axis 0: out[r][c] = P[r][(c - factor r) mod
 * period], where P is `in` followed by zeros up to `period` along the sheared axis. */
int lra_shear_exec(lra_ctx* ctx, const void* in, int esize, int64_t rows_in, int64_t cols_in, int64_t period, int64_t rows_out, int64_t cols_out, int64_t factor, int axis, void* out);
/* feature.stack_memory: in [batch][d][t] -> out [batch][n_steps d][t] of esize-byte elements (device), out[b][step d + i][j] = in[b][i][j - step
 * delay] with np.pad's `mode` (LRA_STACK_*) applied to the column index; LRA_STACK_CONSTANT stores the low esize bytes of `fill`. */
int lra_stack_memory_exec(lra_ctx* ctx, const void* in, int esize, int64_t batch, int64_t d, int64_t t, int64_t n_steps, int64_t delay, int mode, uint64_t fill, void* out);

/* ---- the back half of pyin around the decode: librosa.pyin, librosa/core/pitch.py:796-852 and __pyin_helper :855-931 ---------------------- */
#define LRA_PYIN_LDS_MAX (160 * 1024)
/* Bytes of LDS a workgroup of lra_pyin_obs_exec needs (host arithmetic only): per frame the voiced row (8 n_pitch_bins) and two counters per
 * threshold (8 n_thresholds), four frames per workgroup, halved until they fit; above LRA_PYIN_LDS_MAX the call is refused (LRA_EINVAL). */
int64_t lra_pyin_lds_bytes(int n_pitch_bins, int n_thresholds);
/* cmnd, shifts: float64 [clips][n_lags][n_frames] (device; what lra_yin_exec writes in LRA_YIN_FRAMES mode for float64 samples), never written
 * -> log_prob: float64 [clips][n_frames][2 n_pitch_bins], the layout lra_viterbi_exec reads, holding log(observation_probs + tiny) of
 * __pyin_helper (:870-929); voiced_prob: float64 [clips][n_frames].  Host tables (float64, device): thresholds [n_thresholds] =
 * np.linspace(0, 1, n_thresholds + 1)[1:]; beta_probs [n_thresholds]; beta_prefix [n_thresholds + 1] = np.sum(beta_probs[:m]); boltz_e
 * [n_lags + 1] = exp(-lambda k); boltz_fact [n_lags + 1] = (1 - exp(-lambda)) / (1 - exp(-lambda N)) (scipy's boltzmann._pmf is
 * boltz_fact[N] * boltz_e[k]).  A zero probability stores log_tiny as given. */
int lra_pyin_obs_exec(lra_ctx* ctx, const void* cmnd, const void* shifts, int64_t clips, int n_lags, int64_t n_frames, const void* thresholds, const void* beta_probs,
                      const void* beta_prefix, const void* boltz_e, const void* boltz_fact, int n_thresholds, double sr, double fmin, int min_period, int n_pitch_bins,
                      int n_bins_per_semitone, double no_trough_prob, double tiny, double log_tiny, void* log_prob, void* voiced_prob);
/* states: uint16 [n] (device) -> f0: float64 [n] = freqs[state % n_pitch_bins] (freqs: float64 [n_pitch_bins], device), voiced_flag: one byte per
 * element, state < n_pitch_bins; fill != 0: f0 = fill_na where not voiced (:844-850). */
int lra_pyin_finish_exec(lra_ctx* ctx, const void* states, int64_t n, int n_pitch_bins, const void* freqs, int fill, double fill_na, void* f0, void* voiced_flag);

/* ---- constant-Q / variable-Q transform: librosa.cqt / librosa.vqt, librosa/core/constantq.py:42-225, 820-1122 ---------------------
 * The octave recursion (:1054-1099) is, per octave: lra_stft_exec with a rectangular window (__cqt_response, :1202-1204), then
 * lra_cqt_project_exec (the sparse filter basis applied to every frame, :1213-1218, with the length scaling :1116-1118 and the
 * stacking of __trim_stack :1168-1194 folded in), then lra_fir_decimate_exec (audio.resample by 2, :1095-1098). */

/* out[clip][n] = (sum_k taps[k] x[clip][(n + first) down - k]) / div * mul, x = 0 outside [0, n_in), 0 <= n < n_out.
 * With taps = the zero-prefixed filter, first = n_pre_remove and n_out = ceil(n_in / down) this is
 * scipy.signal.resample_poly(x, 1, down) (librosa/core/audio.py:676-693), summed in its order; div = sqrt(1 / down) is
 * resample(scale=True) (:719-720).  x, out, taps: real of `dtype` (device). */
int lra_fir_decimate_exec(lra_ctx* ctx, const void* x, void* out, int64_t batch, int64_t n_in, int64_t n_out, const void* taps, int n_taps, int down, int first, double div, double mul,
                          int dtype);

/* librosa.resample(res_type="polyphase") for any rational ratio, librosa/core/audio.py:676-693 = scipy.signal.resample_poly(x, up, down):
 * out[clip][n] = (sum_k x[clip][k] taps[(n + first) down - k up]) / div * mul over the real samples k under the filter (the
 * zero-stuffed signal filtered and decimated: scipy's upfirdn, summed in its order).  taps = scipy's design times `up`, zero-prefixed;
 * first = n_pre_remove; n_out = ceil(n_in up / down).  up == 1 is lra_fir_decimate_exec.  x, out, taps: real of `dtype` (device). */
int lra_resample_poly_exec(lra_ctx* ctx, const void* x, void* out, int64_t batch, int64_t n_in, int64_t n_out, const void* taps, int n_taps, int up, int down, int first, double div,
                           double mul, int dtype);

/* librosa.resample(res_type="fft" / "scipy"), librosa/core/audio.py:672-675 = scipy.signal.resample(x, n_out) along the last axis for
 * real x: out[clip] = irfft(Y, n_out) * (n_out / n_in) * gain, Y = the lower min(n_in, n_out) / 2 + 1 bins of rfft(x[clip]) (zero above),
 * the shared Nyquist bin doubled when shortening / halved when lengthening an even length.  Whole-signal transforms (rocFFT, any
 * length < 2^31; plans kept per length, least recently used evicted); gain: the caller's scaling (1 / sqrt(ratio) of
 * resample(scale=True), :719-720).  x: [batch][n_in], out: [batch][n_out] real of `dtype` (device). */
int lra_resample_fft_exec(lra_ctx* ctx, const void* x, void* out, int64_t batch, int64_t n_in, int64_t n_out, double gain, int dtype);

/* Band-limited resampling by a rational ratio in the Fourier domain: the library's own converter behind librosa.resample's soxr_* /
 * kaiser_* / sinc_* names (librosa/core/audio.py:1146-1170; packages that are not in the build image) when the ratio is not a plain
 * decimation.  Each clip is zero-padded to fft_in samples, transformed, multiplied by the low-pass erfc((k - k_mid) / k_sigma) / 2 (bins of
 * the forward transform), cut at the lower Nyquist, inverted at fft_out samples; out[clip] = the first n_out samples * gain * fft_out /
 * fft_in.  The caller chooses fft_in = g down >= n_in + the filter's length and fft_out = g up (then the circular convolution is the linear
 * one and the output grid is exact).  x: [batch][n_in], out: [batch][n_out] real of `dtype` (device). */
int lra_resample_band_exec(lra_ctx* ctx, const void* x, void* out, int64_t batch, int64_t n_in, int64_t n_out, int64_t fft_in, int64_t fft_out, double k_mid, double k_sigma, double gain,
                           int dtype);

/* out[clip][t][bin0 + r] = (sum_j val[j] D[clip][t][col[j]], j in row row0 + r of the CSR basis) / sqrt_len[r], 0 <= r < n_rows,
 * 0 <= t < n_frames.  D: [clip][frames_in][n_bins] complex (lra_stft_exec's layout), out: [clip][n_frames][n_total] complex, both of
 * `dtype`'s precision; row_ptr / col: int32, val: complex (device); sqrt_len: float64 [n_rows] (device) or NULL (scale=False). */
int lra_cqt_project_exec(lra_ctx* ctx, const void* D, void* out, const void* row_ptr, const void* col, const void* val, const void* sqrt_len, int64_t batch, int64_t frames_in, int n_bins,
                         int64_t n_frames, int n_total, int bin0, int row0, int n_rows, int dtype);

/* One octave of the recursion in one launch (round 4): the rectangular-window STFT of centred frames (n_fft a power of two in [32, 4096]:
 * lra_cqt_octave_supported; constantq.py:1197-1212), the sparse basis projection (:1213-1218), the length scaling (:1116-1118) and the stacking
 * (:1168-1194) -- arguments as lra_cqt_project_exec, y [batch][y_stride] instead of D.  The frame spectra stay in LDS.  Raises the context's
 * non-finite flag like the forward kernels (a frame's DC bin is non-finite iff one of its samples is). */
int lra_cqt_octave_supported(int n_fft);
/* The whole octave recursion of one cqt / vqt call in ONE native call (round 5; constantq.py:1054-1099): for every octave lra_cqt_octave_exec on the
 * current signal and -- where `halve` -- lra_fir_decimate_exec by two (taps / first as there, div = sqrt(1/2): audio.resample(scale=True)) into the
 * next slice of `scratch` (>= the sum of the 256-byte-rounded halved signals).  overlap != 0: the octave transforms go to the context's side stream
 * beside the chain of halvings (lra_ctx_side) and are joined before returning.  What the Python loop did with ~40 calls through ctypes per transform. */
typedef struct lra_cqt_octave {
    int n_fft, hop;             /* frame length and hop of the octave's transform */
    int bin0, row0, n_rows;     /* its columns of the stacked result, its rows of the CSR basis */
    int halve;                  /* != 0: the signal is halved behind this octave */
    int64_t n;                  /* samples per clip of the octave's signal */
    const void* row_ptr;        /* CSR basis of the octave (device): int32 row_ptr / col, complex val */
    const void* col;
    const void* val;
} lra_cqt_octave;
int lra_cqt_recursion_exec(lra_ctx* ctx, const void* y, int64_t batch, const lra_cqt_octave* octaves, int n_octaves, int pad_mode, const void* sqrt_len, void* out, int64_t n_frames,
                           int n_total, const void* taps, int n_taps, int first, void* scratch, int64_t scratch_bytes, int overlap, int dtype);
int lra_cqt_octave_exec(lra_ctx* ctx, const void* y, int64_t batch, int64_t n, int64_t y_stride, int n_fft, int hop, int pad_mode, const void* row_ptr, const void* col, const void* val,
                        const void* sqrt_len, void* out, int64_t n_frames, int n_total, int bin0, int row0, int n_rows, int dtype);

/* ---- harmonic / percussive separation: librosa.decompose.hpss, librosa/decompose.py:371-528 (between the stft and the two istft of
 * librosa.effects.hpss / harmonic / percussive, librosa/effects.py:70-301) --------------------------------------------------------- */
/* mag[i] = |D[i]| (np.abs of the complex spectrogram, core/spectrum.py:1347); D complex, mag real of `dtype`'s precision (device). */
int lra_magnitude_exec(lra_ctx* ctx, const void* D, void* mag, int64_t count, int dtype);

/* librosa.magphase, librosa/core/spectrum.py:1296-1361: mag[i] = |D[i]| ** power, phase[i] = D[i] / |D[i]| (1 + 0j where |D[i]| = 0; real and
 * imaginary parts divided separately, :1353-1357).  D: complex (is_complex != 0) or real of `dtype`'s precision; mag real, phase complex
 * (device).  The exponent as NumPy evaluates a scalar one (1, 2, 0.5, -1, 0: copy, square, sqrt, reciprocal, ones; else pow). */
int lra_magphase_exec(lra_ctx* ctx, const void* D, int is_complex, void* mag, void* phase, int64_t count, double power, int dtype);

/* mag: [clip][frame][bin] real (device; |D|, or any non-negative real spectrogram S).  One pass: harm / perc = medians over win_harm
 * frames / win_perc bins (scipy.ndimage.median_filter, mode="reflect", :499-510), the two soft masks (util.softmask with `power`,
 * margins, split_zeros = both margins 1, :512-520; power = inf: hard masks), and
 *   want_mask != 0:  out_h / out_p = the masks (real)                                                          (:522-523)
 *   D == NULL:       out_h / out_p = S * mask (real)                                                            (:528, phase = 1)
 *   else:            out_h / out_p = (|D| * mask) * D / |D| (complex, same layout; phase 1 + 0j where |D| == 0)  (:528, :471-472) */
int lra_hpss_exec(lra_ctx* ctx, const void* mag, const void* D, void* out_h, void* out_p, int64_t batch, int64_t n_frames, int n_bins, int win_harm, int win_perc, double power,
                  double margin_harm, double margin_perc, int want_mask, int dtype);

/* ---- multi-GPU: the trivial gather of the sharded result (the reference has no counterpart) ----------------- */
/* One process per GPU.  Clips shard by contiguous ranges with no collective on the data path; these entry points gather the
 * per-rank results over RCCL (xGMI) for hosts that do not use torch.distributed.  RCCL is bound at run time (dlopen): the
 * library does not depend on it.  Rank 0 obtains an id (LRA_COMM_ID_BYTES bytes) and the host program hands it to the other
 * ranks (MPI, a file, a socket); every rank then creates its communicator on its own context (= device + stream). */
#define LRA_COMM_ID_BYTES 128
typedef struct lra_comm lra_comm;
int lra_comm_unique_id(void* id_out);
int lra_comm_init(lra_ctx* ctx, int rank, int n_ranks, const void* id, lra_comm** out);
/* recv_dev[r * bytes_per_rank ...] = rank r's send_dev[0 .. bytes_per_rank), enqueued on the context's stream (stream-ordered
 * after the kernels that produced send_dev); equal shard sizes -- the shim gathers unequal shards piecewise. */
int lra_comm_allgather(lra_comm* comm, const void* send_dev, void* recv_dev, size_t bytes_per_rank);
/* The same for UNEQUAL shards (clips % ranks != 0: librosa_amd.distributed.shard_range): rank r's bytes_per_rank[r] bytes land at recv_dev + recv_offsets[r] on
 * every rank -- one ncclBroadcast per rank inside one ncclGroupStart / End, no padding, no staging copy.  Both tables are host arrays of n_ranks entries, the same
 * on every rank. */
int lra_comm_allgatherv(lra_comm* comm, const void* send_dev, void* recv_dev, const size_t* bytes_per_rank, const size_t* recv_offsets);
void lra_comm_destroy(lra_comm* comm);

/* ---- measurement aid (no reference counterpart): the transform's access stream without its arithmetic ------------------
 * direction 0: per row read `hop` float32 of PCM and write one row of n_fft/2 + 1 complex64 (the shape of the array
 * librosa/core/spectrum.py:356 allocates); direction 1: read a row, write `hop` samples (the columns :598 reads).  Same
 * decomposition as the fused kernels (one wave64 per strip of `strip_rows` consecutive rows, 8-byte pieces, next row's loads
 * ahead of this row's stores), `waves_per_cu` resident waves per CU (0 = 12, the forward kernel's residency).  bench.py
 * reports it as `stream_ceiling`: what this mix of reads and 8-byte-aligned row writes reaches on the chip at hand
 * (SURVEY.md 8d prices the kernels against 8 TB/s).  n_fft in {256, 512, ..., 2048}, hop a multiple of 128. */
int lra_probe_stream(lra_ctx* ctx, int direction, const void* in, void* out, int64_t batch, int64_t rows_per_clip, int n_fft, int hop, int64_t clip_samples,
                     int strip_rows, int waves_per_cu);
/* ... with the rows `row_pitch_bytes` apart (0 = packed: (n_fft/2 + 1) * 8; a multiple of 8) and the row side moved in pieces of
 * `piece_bytes`: 8 = the kernels' own butterfly order (bins k ascending from one base, M - k descending from the other), 16 = wave-wide
 * 1 KiB pieces in address order + bin M (needs a pitch that is a multiple of 16). */
int lra_probe_stream_pitched(lra_ctx* ctx, int direction, const void* in, void* out, int64_t batch, int64_t rows_per_clip, int n_fft, int hop, int64_t clip_samples,
                             int strip_rows, int waves_per_cu, int64_t row_pitch_bytes, int piece_bytes);

/* ... the forward stream with strips of `strip_rows` rows dealt out in address order to n_cu x waves_per_cu persistent waves (all of them writing
 * inside one moving window of the result): the locality experiment of profiles/r05_pitch.md. */
int lra_probe_stream_window(lra_ctx* ctx, const void* in, void* out, int64_t batch, int64_t rows_per_clip, int n_fft, int hop, int64_t clip_samples, int strip_rows, int waves_per_cu);

/* ---- layout helper: dst[b][c][r] = src[b][r][c], elem_bytes in {4, 8, 16} ------------------ */
int lra_transpose(lra_ctx* ctx, const void* src, void* dst, int64_t batch, int64_t rows, int64_t cols, int elem_bytes);

#ifdef __cplusplus
}
#endif
#endif /* LIBROSA_AMD_H */
