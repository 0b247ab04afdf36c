"""``stft`` / ``istft`` / ``_spectrogram`` with librosa's signatures, executed on MI355X.

Host side of the drop-in boundary: argument defaults, validation, warnings and
error types follow ``librosa/core/spectrum.py`` (``stft`` :57-391, ``istft`` :394-626,
``_spectrogram`` :2920-3015) and run BEFORE any device work; the arithmetic itself is done by the
gfx950 library through ``librosa_amd._native`` (fused LDS-FFT kernels for power-of-two ``n_fft``,
rocFFT otherwise).  There is no CPU fallback.

Extensions beyond the reference (which only accepts ``np.ndarray``):
  * ``y`` / ``stft_matrix`` may be a ``torch`` tensor resident on a ROCm device; a device tensor is
    returned and nothing crosses PCIe.  ``check_finite`` then controls the ``valid_audio`` scan.
"""
from __future__ import annotations

import collections
import os
import functools
import threading
import warnings

import numpy as np

from .. import _arrays
from .. import filters
from ..util import utils as util
from ..util.exceptions import ParameterError
from ..util.utils import is_torch_tensor

__all__ = ["stft", "istft", "_spectrogram", "magphase", "griffinlim", "phase_vocoder", "power_to_db", "amplitude_to_db", "db_to_power", "db_to_amplitude"]

# np.pad modes that do not depend only on edge values: rejected exactly as the reference does
_REJECTED_PAD_MODES = ("wrap", "maximum", "mean", "median", "minimum")
# pad modes the framing kernel evaluates on the fly; anything else is pre-padded by np.pad
_DEVICE_PAD_MODES = ("constant", "reflect", "edge", "symmetric")


def _real_compute_dtype(in_dtype, out_complex_dtype):
    """Precision the device computes in: f64 if either side is double, else f32."""
    if np.dtype(in_dtype) == np.float64 or np.dtype(out_complex_dtype) == np.complex128:
        return np.dtype(np.float64)
    return np.dtype(np.float32)


def _validate_audio(y, check_finite):
    """``util.valid_audio`` (``util/utils.py:294-306``) for ndarrays; dtype/ndim checks for tensors.

    Returns True when the finite-scan still has to be done on the device (tensor inputs)."""
    if is_torch_tensor(y):
        if not y.is_floating_point():
            raise ParameterError("Audio data must be floating-point")
        if y.ndim == 0:
            raise ParameterError(f"Audio data must be at least one-dimensional, given y.shape={tuple(y.shape)}")
        return bool(check_finite)
    util.valid_audio(y, scan=False)  # type / rank checks now; the finite scan rides on the staging copy (lra_stft_exec_host)
    return True


def _all_finite(y):
    return bool(_arrays._torch().isfinite(y).all()) if is_torch_tensor(y) else bool(np.isfinite(y).all())


def _direct_out(out, n_frames, n_bins, dtype):
    """``out=`` of ``stft``: (target, pointer-able base, item stride in reals) when the kernels' [frame][bin] layout can be
    written into ``out`` in place -- i.e. ``out`` is laid out like the array ``stft`` itself returns (each frame's
    spectrum contiguous, ``core/spectrum.py:356``), possibly with more columns than needed -- else (target, None, 0)."""
    target = out if out.shape[-1] == n_frames else out[..., :n_frames]
    if out.dtype == np.dtype(dtype) and np.swapaxes(out, -1, -2).flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]:
        return target, out, int(out.shape[-1]) * n_bins * 2
    return target, None, 0


def _prepare_stft(y, n_fft, hop_length, win_length, window, center, pad_mode, _warn_level=4):
    """Shared front end of stft/_spectrogram/melspectrogram: defaults, checks, window, padding.

    Returns (y, hop_length, fft_window (float64, length n_fft), center, pad_mode)."""
    if win_length is None:
        win_length = n_fft
    if hop_length is None:
        hop_length = int(win_length // 4)
    elif not util.is_positive_int(hop_length):
        raise ParameterError(f"hop_length={hop_length} must be a positive integer")
    if not util.is_positive_int(n_fft):
        raise ParameterError(f"n_fft={n_fft} must be a positive integer")
    fft_window = _padded_window(window, win_length, n_fft)
    n = y.shape[-1]
    if center:
        if pad_mode in _REJECTED_PAD_MODES:
            raise ParameterError(f"pad_mode='{pad_mode}' is not supported by librosa.stft")
        if n_fft > n:
            warnings.warn(f"n_fft={n_fft} is too large for input signal of length={n}", stacklevel=_warn_level)
        if not (isinstance(pad_mode, str) and pad_mode in _DEVICE_PAD_MODES):
            # exotic np.pad modes (linear_ramp, empty, callables, ...): pad on the host, then run uncentred
            if is_torch_tensor(y):
                raise ParameterError(f"pad_mode={pad_mode!r} is only supported for numpy inputs")
            widths = [(0, 0)] * y.ndim
            widths[-1] = (n_fft // 2, n_fft // 2)
            y = np.pad(y, widths, mode=pad_mode)
            center, pad_mode = False, "constant"
    else:
        if n_fft > n:
            raise ParameterError(f"n_fft={n_fft} is too large for uncentered analysis of input signal of length={n}")
        pad_mode = "constant"
    return y, int(hop_length), fft_window, bool(center), pad_mode


@functools.lru_cache(maxsize=64)
def _padded_window_cached(window, win_length, n_fft):
    w = util.pad_center(np.asarray(filters.get_window(window, win_length, fftbins=True), dtype=np.float64), size=n_fft)
    w.setflags(write=False)
    return w


def _padded_window(window, win_length, n_fft):
    """``pad_center(get_window(window, win_length, fftbins=True), n_fft)`` in float64 (``core/spectrum.py:240-246``), memoised
    for hashable window specifications (names, tuples); arrays and callables are evaluated every time."""
    if isinstance(window, (str, tuple, float, int)):
        try:
            return _padded_window_cached(window, int(win_length), int(n_fft))
        except TypeError:
            pass
    return util.pad_center(np.asarray(filters.get_window(window, win_length, fftbins=True), dtype=np.float64), size=n_fft)


class _ByteBoundedLRU:
    """Memo of host arrays bounded by entry count AND by bytes (a window sum-square envelope has one value per output sample: an
    entry-count bound alone let 32 hour-long envelopes hold ~10 GB of RAM).  Arrays above a quarter of the budget are not kept."""

    def __init__(self, max_entries, max_bytes):
        self.max_entries, self.max_bytes = int(max_entries), int(max_bytes)
        self._d = collections.OrderedDict()
        self._lock = threading.Lock()

    def get(self, key, build):
        with self._lock:
            hit = self._d.get(key)
            if hit is not None:
                self._d.move_to_end(key)
                return hit
        val = build()
        if val.nbytes <= self.max_bytes // 4:
            with self._lock:
                self._d[key] = val
                while len(self._d) > 1 and (len(self._d) > self.max_entries or sum(v.nbytes for v in self._d.values()) > self.max_bytes):
                    self._d.popitem(last=False)
        return val

    def nbytes(self):
        with self._lock:
            return sum(v.nbytes for v in self._d.values())

    def clear(self):
        with self._lock:
            self._d.clear()


_WSS_CACHE = _ByteBoundedLRU(max_entries=8, max_bytes=128 << 20)


def _istft_wss_cached(window, n_frames, win_length, n_fft, hop, center, expected, out_dtype, real):
    def build():
        wss = filters.window_sumsquare(window=window, n_frames=n_frames, win_length=win_length, n_fft=n_fft, hop_length=hop, dtype=np.dtype(out_dtype))
        wss = np.ascontiguousarray(util.fix_length(wss[(n_fft // 2 if center else 0) :], size=expected), dtype=np.dtype(real))
        wss.setflags(write=False)
        return wss

    key = (window, n_frames, win_length, n_fft, hop, center, expected, out_dtype, real)
    hash(key)  # (an unhashable window specification raises TypeError here: the caller computes without the memo)
    return _WSS_CACHE.get(key, build)


def _istft_wss(window, n_frames, win_length, n_fft, hop, center, expected, out_dtype, real):
    """The inverse transform's window sum-square envelope, computed on the host in the output precision exactly as the reference does
    (``core/spectrum.py:606-620``: ``window_sumsquare`` -> drop the centre padding -> ``fix_length``), and the key under which a context
    may keep its device copy (None for window specifications that cannot be hashed).  The envelope depends on the arguments only; its
    O(n_frames x n_fft) fill loop is 2-8 ms on a host core, which dwarfed the 0.1 ms kernel of a 32-clip device-resident call."""
    args = (int(n_frames), int(win_length), int(n_fft), int(hop), bool(center), int(expected), np.dtype(out_dtype).str, np.dtype(real).str)
    if isinstance(window, (str, tuple, float, int)):
        try:
            return _istft_wss_cached(window, *args), ("istft_wss", window) + args
        except TypeError:
            pass
    wss = filters.window_sumsquare(window=window, n_frames=n_frames, win_length=win_length, n_fft=n_fft, hop_length=int(hop), dtype=out_dtype)
    return np.ascontiguousarray(util.fix_length(wss[(n_fft // 2 if center else 0) :], size=int(expected)), dtype=real), None


# Clips are independent (the reference asserts batch == per item, tests/test_multichannel.py:96-111), so a NumPy batch splits into
# contiguous clip ranges with nothing exchanged between them: one range per visible device, each through that device's own context and
# native host pipeline, from its own thread.  Below this much host data per device the extra contexts are not worth waking up.
_MULTI_DEVICE_MIN_BYTES = 8 << 20


def _sharded_host_exec(sess, batch, nbytes, run):
    """``run(ctx, b, e)`` pushes clips ``[b, e)`` through ``ctx``'s host pipeline (plans are looked up per context) and returns its
    non-finite flag.  With one device -- or a small job -- this is ``run(sess.ctx, 0, batch)``.  With several (``_native.host_devices()``,
    env ``LRA_DEVICES``) device i takes ``shard_range(batch, i, n)``: the calling thread serves the session's own device, one thread per
    further device serves the rest; the first exception is re-raised after every thread has finished."""
    from .. import _native
    from ..distributed import shard_range

    devs = _native.host_devices()
    if len(devs) <= 1 or batch < 2 * len(devs) or nbytes < _MULTI_DEVICE_MIN_BYTES * len(devs):
        if len(devs) == 1 and devs[0] != sess.ctx.device:  # LRA_DEVICES names ONE device that is not the session's: the whole call goes there
            ctx = _native.get_context(devs[0])
            with ctx.call_lock:
                ctx.use_own_stream()
                return run(ctx, 0, batch)
        return run(sess.ctx, 0, batch)
    by_dev = collections.OrderedDict()
    for i, d in enumerate(devs):
        b, e = shard_range(batch, i, len(devs))
        if e > b:
            by_dev.setdefault(d, []).append((b, e))
    flags, errors = [], []

    def serve(ctx, ranges, lock):
        try:
            if lock:
                ctx.call_lock.acquire()
            try:
                if lock:
                    ctx.use_own_stream()
                for b, e in ranges:
                    flags.append(bool(run(ctx, b, e)))
            finally:
                if lock:
                    ctx.call_lock.release()
        except BaseException as exc:  # noqa: BLE001 - re-raised on the calling thread
            errors.append(exc)

    threads = []
    mine = by_dev.pop(sess.ctx.device, [])
    for d, ranges in by_dev.items():
        th = threading.Thread(target=serve, args=(_native.get_context(d), ranges, True), name=f"lra-dev{d}", daemon=True)
        th.start()
        threads.append(th)
    serve(sess.ctx, mine, False)  # (the session already holds this context's lock and selected its stream)
    for th in threads:
        th.join()
    if errors:
        raise errors[0]
    return any(flags)


# A batch with fewer clips than devices cannot shard by clips; ONE long clip (hours of audio: SURVEY.md 8(e), the reference's own answer is block-wise
# `stream`, core/audio.py:223-533) shards by FRAMES instead: device i takes frames shard_range(n_frames, i, n) of every clip, computed as the uncentred
# transform of its sample range plus the n_fft - hop halo, the centre padding going to the first / last shard (distributed.shard_frames).  Same
# opt-in as the clip sharding (LRA_DEVICES); below this many frames per device it is not worth it.
_FRAME_SHARD_MIN_FRAMES = 256


def _frame_shard_plan(n, n_frames, batch, nbytes, n_fft, hop, center):
    """[(device, shard)] when this call is to be sharded by frames, else None."""
    from .. import _native
    from ..distributed import shard_frames, split_padded_edges

    devs = _native.host_devices()
    if len(devs) <= 1 or batch >= 2 * len(devs) or batch < 1:
        return None
    if n_frames < _FRAME_SHARD_MIN_FRAMES * len(devs) or nbytes < _MULTI_DEVICE_MIN_BYTES * len(devs):
        return None
    pad = n_fft // 2 if center else 0
    if n < 2 * pad + 2:  # (centre padding longer than the clip: repeated reflection does not split)
        return None
    shards = [(d, shard_frames(n, i, len(devs), n_fft, hop, center)) for i, d in enumerate(devs)]
    # (the frames that touch the centre padding run on their own: the padded copy is then a frame or two long, the rest of an edge shard a view)
    return [(d, run) for d, sh in shards if sh["frame_hi"] > sh["frame_lo"] for run in split_padded_edges(n, sh, n_fft, hop, center)]


def _istft_sample_shards(expected, n_used, batch, nbytes, n_fft, hop, center):
    """[(device, (s0, s1, fa, fb))]: output samples [s0, s1) of the final signal and the frames [fa, fb) that reach into them; None = do not shard."""
    from .. import _native
    from ..distributed import shard_range

    devs = _native.host_devices()
    if len(devs) <= 1 or batch >= 2 * len(devs) or batch < 1 or n_used < _FRAME_SHARD_MIN_FRAMES * len(devs) or nbytes < _MULTI_DEVICE_MIN_BYTES * len(devs):
        return None
    drop = n_fft // 2 if center else 0
    out = []
    for i, d in enumerate(devs):
        s0, s1 = shard_range(expected, i, len(devs))
        if s1 <= s0:
            continue
        u0, u1 = s0 + drop, s1 + drop  # positions in the untrimmed overlap-add buffer
        fa = max(0, (u0 - n_fft) // hop + 1)
        fb = min(n_used, (u1 - 1) // hop + 1)
        if fb <= fa:  # samples beyond the last frame (length= longer than the frames reach): zeros, left to the unsharded call's semantics
            return None
        out.append((d, (s0, s1, fa, fb)))
    return out


def _frame_sharded_host_exec(sess, shards, run):
    """``run(ctx, shard)`` for every (device, shard), the session's own device on the calling thread and one thread per further device (several shards
    of one device run one after the other on its thread); returns whether any shard saw a non-finite sample."""
    from .. import _native

    by_dev = collections.OrderedDict()
    for d, sh in shards:
        by_dev.setdefault(d, []).append(sh)
    flags, errors = [], []

    def serve(ctx, items, lock):
        try:
            if lock:
                ctx.call_lock.acquire()
            try:
                if lock:
                    ctx.use_own_stream()
                for sh in items:
                    flags.append(bool(run(ctx, sh)))
            finally:
                if lock:
                    ctx.call_lock.release()
        except BaseException as exc:  # noqa: BLE001 - re-raised on the calling thread
            errors.append(exc)

    mine = by_dev.pop(sess.ctx.device, [])
    threads = []
    for d, items in by_dev.items():
        th = threading.Thread(target=serve, args=(_native.get_context(d), items, True), name=f"lra-dev{d}", daemon=True)
        th.start()
        threads.append(th)
    serve(sess.ctx, mine, False)
    for th in threads:
        th.join()
    if errors:
        raise errors[0]
    return any(flags)


def wss_to_norm(wss):
    """Window sum-square envelope -> the factors the inverse kernels multiply by: ``1 / wss`` where ``wss > tiny(wss)``, else 1 -- the
    reference's ``y[approx_nonzero_indices] /= ifft_window_sum[approx_nonzero_indices]`` (``core/spectrum.py:622-624``) as a product, in the
    envelope's own precision (each factor correctly rounded; the product is within 1 ulp of the division)."""
    wss = np.asarray(wss)
    one = wss.dtype.type(1)
    with np.errstate(divide="ignore", over="ignore"):
        return np.where(wss > util.tiny(wss), one / wss, one).astype(wss.dtype, copy=False)


def _device_norm(sess, wss, wss_key, real):
    """Device pointer of the normalisation factors of ``wss`` (memoised per context under the envelope's key, in the byte-bounded pool)."""
    ctx = sess.ctx
    if wss_key is not None and ctx.table_cacheable(wss.nbytes, "large"):
        return ctx.device_table(("norm",) + tuple(wss_key), lambda: wss_to_norm(wss), pool="large")
    return sess.input_raw(_as_like(sess, wss_to_norm(wss)), real)


# Optional (LRA_ROW_ALIGN bytes, default 0 = packed; per call: stft(..., row_align=128)): the rows of a device-resident complex / power result padded
# to whole 128-byte cache lines behind the (..., n_bins, n_frames) view -- the reference's own result is such a strided view (order="F",
# core/spectrum.py:356), only stride(-1) becomes row_pitch instead of n_bins.  VERDICT r04 proposed it as the way to a faster store stream; measured
# in round 5 it is NOT one: on the same allocation the padded layout is 1-6 % SLOWER than packed rows (0.661 vs 0.647, 0.777 vs 0.745 ms for the
# 2048 / 512 transform), and what first looked like a 13 % gain was the placement of the output allocation, which moves the same kernel between
# 0.633 and 0.745 ms inside one process (profiles/r05_pitch.md).  Kept as an option (istft, melspectrogram(S=...) and the frame-major consumers
# take such views in place); off by default.
ROW_ALIGN_BYTES = int(os.environ.get("LRA_ROW_ALIGN", "0") or 0)
_ROW_ALIGN_MIN_ROW_BYTES = 4096   # rows shorter than this are never padded


def row_pitch(n_bins, itemsize, align=None):
    """Elements between the rows of consecutive frames in a device-resident result of ``stft`` / ``_spectrogram``."""
    align = ROW_ALIGN_BYTES if align is None else int(align)
    if align <= 0 or n_bins * itemsize < _ROW_ALIGN_MIN_ROW_BYTES or align % itemsize:
        return int(n_bins)
    per = align // itemsize
    return int((n_bins + per - 1) // per * per)


def _frame_major_strides(xt, n_bins):
    """(batch stride, frame stride) in elements when the tensor ``xt`` of shape (..., n_frames, n_bins) can be walked as [batch][frame][bin] in
    place -- bins contiguous, frames a fixed distance >= n_bins apart, the leading axes collapsing into one -- else None."""
    if xt.ndim < 2 or xt.shape[-1] != n_bins or (n_bins > 1 and xt.stride(-1) != 1):
        return None
    fs = int(xt.stride(-2)) if xt.shape[-2] > 1 else int(n_bins)
    if fs < n_bins:
        return None
    bs = fs * int(xt.shape[-2])
    if xt.ndim > 2:
        lead = [(int(sz), int(st)) for sz, st in zip(xt.shape[:-2], xt.stride()[:-2]) if sz > 1]
        if lead:
            bs = lead[-1][1]
            if bs < fs * int(xt.shape[-2]):
                return None
            for (sz0, st0), (sz1, st1) in zip(lead[:-1], lead[1:]):
                if st0 != st1 * sz1:
                    return None
    return bs, fs


def _finite_check_covers_input(n, n_fft, hop, center):
    """True when every input sample lies in some frame, so the kernels' DC-bin flag sees it."""
    if hop > n_fft:
        return False
    padded = n + (2 * (n_fft // 2) if center else 0)
    n_frames = 1 + (padded - n_fft) // hop
    covered_hi = (n_frames - 1) * hop + n_fft  # exclusive, padded coordinates
    return covered_hi >= (n + (n_fft // 2 if center else 0))


def _run_stft_family(kind, y, *, n_fft, hop_length, win_length, window, center, pad_mode, dtype=None, power=1.0, mel_basis=None, check_finite=True, post=None, out=None,
                     row_align=None):
    """kind in {"stft", "power", "mel"}.  Returns the result laid out like the reference's.

    ``post(sess, mel_ptr, batch, n_mels, n_frames, real) -> (handle, rows)`` (mel only) chains further device work on the mel
    spectrogram before anything is downloaded (``feature.mfcc``); the result then has ``rows`` rows instead of ``n_mels``.  ``post`` may
    return ``(handle, rows, cols)`` when its result has ``cols`` columns instead of ``n_frames`` (``onset.onset_strength_multi``).

    With ``kind="power"`` the hook is ``post(sess, s_ptr, batch, n_bins, n_frames, pitch, real) -> (handle, rows)``: ``s_ptr`` is the power
    spectrogram [batch][n_frames][pitch] on the device (``pitch >= n_bins`` elements between the rows of consecutive frames); the spectrogram is
    not downloaded and the result is the ``(..., rows, n_frames)`` array of ``handle`` (``feature.chroma_stft``), or, with ``rows`` None, the
    array of ``handle`` as the hook shaped it (``piptrack``, ``estimate_tuning``)."""
    need_device_check = _validate_audio(y, check_finite)
    y, hop, fft_window, center, pad_mode = _prepare_stft(y, n_fft, hop_length, win_length, window, center, pad_mode)
    in_dtype = _arrays.numpy_dtype_of(y)
    if kind == "stft":
        out_dtype = np.dtype(util.dtype_r2c(in_dtype)) if dtype is None else np.dtype(dtype)
        if out_dtype.kind != "c":
            raise ParameterError(f"stft dtype={out_dtype} is not of complex type")
        real = _real_compute_dtype(in_dtype, out_dtype)
    else:
        real = np.dtype(np.float64) if in_dtype == np.float64 else np.dtype(np.float32)
        if kind == "mel" and np.dtype(mel_basis.dtype) == np.float64:
            real = np.dtype(np.float64)
    lead = tuple(y.shape[:-1])
    n = int(y.shape[-1])
    n_bins = 1 + n_fft // 2
    sess = _arrays.Session(y)
    try:
        ctx = sess.ctx
        plan = ctx.stft_plan(n_fft, hop, fft_window.astype(real), center, pad_mode, real)
        n_frames = ctx.stft_num_frames(plan, n)
        fused = ctx.stft_is_fused(plan)
        if out is not None:  # shape / dtype checks of core/spectrum.py:357-367, before any work
            shape = list(lead) + [n_bins, n_frames]
            if not (np.allclose(out.shape[:-1], shape[:-1]) and out.shape[-1] >= shape[-1]):
                raise ParameterError(f"Shape mismatch for provided output array out.shape={out.shape} and target shape={shape}")
            if not np.iscomplexobj(out):
                raise ParameterError(f"output with dtype={out.dtype} is not of complex type")
        host_pipeline = not sess.is_torch and post is None
        if need_device_check and not host_pipeline:
            if fused and _finite_check_covers_input(n, n_fft, hop, center):
                ctx.nonfinite_reset()
            else:
                need_device_check = False
                if not _all_finite(y):
                    raise ParameterError("Audio buffer is not finite everywhere")
        if host_pipeline:
            # NumPy in, NumPy out: the native host pipeline (chunked, overlapped staging; include/librosa_amd.h)
            a = np.ascontiguousarray(y, dtype=real).reshape(-1, n)
            batch = a.shape[0]
            if batch == 0:  # no clips (y.shape == (0, n)): the reference returns an empty array of the result's shape and dtype
                if kind == "mel":
                    return np.empty(lead + (int(mel_basis.shape[0]), n_frames), dtype=real)
                empty = np.empty(lead + (n_bins, n_frames), dtype=out_dtype if kind == "stft" else real)
                return out[..., :n_frames] if out is not None else empty
            target, stride = None, 0
            if kind == "stft":
                cdt = np.dtype(util.dtype_r2c(real))
                if out is not None:
                    target, base, stride = _direct_out(out, n_frames, n_bins, cdt)
                    host = base
                if out is None or base is None:
                    host, stride = np.empty((batch, n_frames, n_bins), dtype=cdt), 0
            elif kind == "power":
                host = np.empty((batch, n_frames, n_bins), dtype=real)
            else:
                n_mels = int(mel_basis.shape[0])
                basis = np.ascontiguousarray(mel_basis, dtype=real)
                host = np.empty((batch, n_mels, n_frames), dtype=real)
            win = fft_window.astype(real)
            item_out = stride * real.itemsize if stride else host[0].size * host.itemsize  # bytes between the results of consecutive clips (`stride` counts reals)

            def run(c, b, e):
                pl = plan if c is ctx else c.stft_plan(n_fft, hop, win, center, pad_mode, real)
                mp = c.mel_plan(basis) if kind == "mel" else None
                return c.stft_exec_host(pl, mp, {"stft": 0, "power": 1, "mel": 2}[kind], a.ctypes.data + b * n * a.itemsize, e - b, n, n, power,
                                        host.ctypes.data + b * item_out, stride)

            fshards = _frame_shard_plan(n, n_frames, batch, a.nbytes + host.nbytes, n_fft, hop, center)
            if fshards is not None:
                from ..distributed import frame_shard_input

                def run_frames(c, sh):
                    # the shard's frames = the UNCENTRED frames of its sample range (+ its share of the centre padding): distributed.shard_frames
                    piece = frame_shard_input(a, sh, pad_mode)
                    m, f0, nf = int(piece.shape[-1]), sh["frame_lo"], sh["frame_hi"] - sh["frame_lo"]
                    pl = c.stft_plan(n_fft, hop, win, False, "constant", real)
                    assert c.stft_num_frames(pl, m) == nf
                    y_stride = piece.strides[0] // piece.itemsize if piece.ndim == 2 and piece.shape[0] > 1 else m
                    if kind == "mel":
                        part = np.empty((batch, n_mels, nf), dtype=real)
                        flag = c.stft_exec_host(pl, c.mel_plan(basis), 2, piece.ctypes.data, batch, m, y_stride, power, part.ctypes.data, 0)
                        host[:, :, f0 : f0 + nf] = part
                        return flag
                    per_frame = n_bins * (2 if kind == "stft" else 1)  # reals per frame row
                    item = stride if stride else n_frames * per_frame   # reals between the results of consecutive clips
                    return c.stft_exec_host(pl, None, 0 if kind == "stft" else 1, piece.ctypes.data, batch, m, y_stride, power,
                                            host.ctypes.data + f0 * per_frame * real.itemsize, item)

                flagged = _frame_sharded_host_exec(sess, fshards, run_frames)
            else:
                flagged = _sharded_host_exec(sess, batch, a.nbytes + host.nbytes, run)
            if flagged:  # util.valid_audio's scan (util/utils.py:305), done by the staging threads on the samples they copy
                raise ParameterError("Audio buffer is not finite everywhere")
            if kind == "mel":
                return host.reshape(lead + (n_mels, n_frames))
            if target is not None:
                if host is not out:
                    target[...] = _arrays.swap_last_two(host.reshape(lead + (n_frames, n_bins)))
                return target
            res = _arrays.swap_last_two(host.reshape(lead + (n_frames, n_bins)))
            return _arrays.cast(res, out_dtype) if kind == "stft" else res
        y_ptr, batch, _, y_stride = sess.input_2d(y, real)
        pitch = n_bins
        if kind != "mel" and sess.is_torch and fused:  # device-resident result: rows padded to whole cache lines behind the view (see row_pitch)
            pitch = row_pitch(n_bins, np.dtype(util.dtype_r2c(real) if kind == "stft" else real).itemsize, row_align)
        if kind == "stft":
            ptr, handle = sess.output((batch, n_frames, pitch), util.dtype_r2c(real), rows=True)
            if pitch == n_bins:
                ctx.stft_exec(plan, y_ptr, batch, n, y_stride, ptr)
            else:
                ctx.stft_exec_strided(plan, 0, y_ptr, batch, n, y_stride, 1.0, ptr, pitch)
        elif kind == "power":
            ptr, handle = sess.output((batch, n_frames, pitch), real, rows=True)
            if pitch == n_bins:
                ctx.spectrogram_exec(plan, y_ptr, batch, n, y_stride, power, ptr)
            else:
                ctx.stft_exec_strided(plan, 1, y_ptr, batch, n, y_stride, power, ptr, pitch)
            if post is not None:
                if not sess.is_torch:
                    sess._keep.append(handle[0])  # the spectrogram itself is not downloaded
                handle, post_rows = post(sess, ptr, batch, n_bins, n_frames, pitch, real)
        else:
            n_mels = int(mel_basis.shape[0])
            mel_plan = ctx.mel_plan(np.ascontiguousarray(mel_basis, dtype=real))
            ptr, handle = sess.output((batch, n_mels, n_frames), real)
            ctx.melspectrogram_exec(plan, mel_plan, y_ptr, batch, n, y_stride, power, ptr)
            if post is not None:
                handle, n_mels, *cols = post(sess, ptr, batch, n_mels, n_frames, real)
                if cols:
                    n_frames = int(cols[0])
        if need_device_check and ctx.nonfinite_read():
            # the flag says "some frame's DC bin is not finite"; finite samples of enormous magnitude overflow it
            # too, so the samples themselves decide (util.valid_audio tests np.isfinite(y), util/utils.py:305)
            if not _all_finite(y):
                raise ParameterError("Audio buffer is not finite everywhere")
        res = sess.result(handle)
    finally:
        sess.close()
    if kind == "mel":
        return res.reshape(lead + (n_mels, n_frames))
    if kind == "power" and post is not None:
        return res if post_rows is None else res.reshape(lead + (int(post_rows), n_frames))
    if pitch != n_bins:
        res = res.view(lead + (n_frames, pitch))[..., :n_bins]  # the padding stays behind the view
    res = _arrays.swap_last_two(res.reshape(lead + (n_frames, n_bins)))  # (..., n_bins, n_frames) view
    if kind == "stft":
        res = _arrays.cast(res, out_dtype)
    return res


def stft(y, *, n_fft=2048, hop_length=None, win_length=None, window="hann", center=True, dtype=None, pad_mode="constant", out=None,
         check_finite=True, row_align=None):
    """Short-time Fourier transform; drop-in for ``librosa.stft`` (``librosa/core/spectrum.py:57-391``).

    Returns ``D[..., f, t]`` of shape ``(..., 1 + n_fft//2, n_frames)``, complex64 for float32 audio and
    complex128 for float64 (or ``dtype``).  As in the reference (which allocates Fortran-ordered,
    ``:356``) each frame's spectrum is contiguous in memory: the array is a transposed view of the
    device layout ``[..., t, f]``.

    ``out`` (numpy only): a pre-allocated complex array with matching leading shape and at least
    ``n_frames`` columns; the same object (or ``out[..., :n_frames]``) is returned (``:355-367``).

    Device tensors (extension): ``row_align=128`` (default ``LRA_ROW_ALIGN`` = 0: packed rows) starts each frame's row of the result on a
    128-byte boundary -- ``stride(-1)`` of the returned view is then ``row_pitch(n_bins, itemsize, 128)`` rather than ``n_bins``; shape, dtype
    and values are the same, ``.contiguous()`` compacts, and ``istft`` reads the view in place.  Measured in round 5: no faster than packed rows
    (``profiles/r05_pitch.md``), hence off by default.
    """
    if out is not None and is_torch_tensor(y):
        raise ParameterError("out= is only supported for numpy inputs")
    return _run_stft_family("stft", y, n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window, center=center, pad_mode=pad_mode,
                            dtype=dtype if out is None else (dtype or util.dtype_r2c(_arrays.numpy_dtype_of(y))), check_finite=check_finite, out=out, row_align=row_align)


def _spectrogram(*, y=None, S=None, n_fft=2048, hop_length=512, power=1, win_length=None, window="hann", center=True, pad_mode="constant"):
    """``librosa.core.spectrum._spectrogram`` (``librosa/core/spectrum.py:2920-3015``).

    With ``S`` given, only ``n_fft`` is inferred; otherwise ``S = |stft(y)|**power`` is produced by the
    fused kernel (magnitude/power taken in registers, the complex spectrum never reaches HBM).
    """
    if S is not None:
        if n_fft is None or n_fft // 2 + 1 != S.shape[-2]:
            n_fft = 2 * (S.shape[-2] - 1)
        return S, n_fft
    if n_fft is None:
        raise ParameterError(f"Unable to compute spectrogram with n_fft={n_fft}")
    if y is None:
        raise ParameterError("Input signal must be provided to compute a spectrogram")
    S = _run_stft_family("power", y, n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window, center=center, pad_mode=pad_mode,
                         power=float(power))
    return S, n_fft


def _istft_frame_counts(n_total_frames, n_fft, hop_length, center, length):
    """Frame bookkeeping of ``librosa/core/spectrum.py:523-544, 557-603``.

    Returns (n_frames for the window-sum-square, n_used frames that contribute, expected length)."""
    if length:
        padded_length = length + 2 * (n_fft // 2) if center else length
        n_frames = min(n_total_frames, int(np.ceil(padded_length / hop_length)))
    else:
        n_frames = n_total_frames
    expected = n_fft + hop_length * (n_frames - 1)
    if length:
        expected = length
    elif center:
        expected -= 2 * (n_fft // 2)
    if center:
        # the reference always folds the first ceil((n_fft/2)/hop) frames in through its head block
        start_frame = int(np.ceil((n_fft // 2) / hop_length))
        n_used = max(n_frames, min(n_total_frames, start_frame))
    else:
        n_used = n_frames
    return n_frames, n_used, expected


def istft(stft_matrix, *, hop_length=None, win_length=None, n_fft=None, window="hann", center=True, dtype=None, length=None, out=None):
    """Inverse STFT; drop-in for ``librosa.istft`` (``librosa/core/spectrum.py:394-626``).

    Frames are inverse-transformed, windowed and overlap-added in frame order, then divided by the
    window sum-square envelope wherever it exceeds ``tiny`` (``:606-624``).  ``length`` trims/zero-pads
    the output and limits the frames used (``:523-531``).
    """
    D = stft_matrix
    if D.ndim < 2:
        raise ParameterError(f"stft_matrix must have at least 2 dimensions, given shape={tuple(D.shape)}")
    if n_fft is None:
        n_fft = 2 * (D.shape[-2] - 1)
    if D.shape[-2] != 1 + n_fft // 2:
        # an explicit n_fft that disagrees with the matrix: scipy's irfft(n=n_fft) (core/spectrum.py:566,598) crops
        # the bin axis to 1 + n_fft//2 or zero-pads it, and so does the drop-in
        D = _fit_bins(D, 1 + n_fft // 2)
    if win_length is None:
        win_length = n_fft
    if hop_length is None:
        hop_length = int(win_length // 4)
    elif not util.is_positive_int(hop_length):
        raise ParameterError(f"hop_length={hop_length} must be a positive integer")
    ifft_window = util.pad_center(np.asarray(filters.get_window(window, win_length, fftbins=True), dtype=np.float64), size=n_fft)
    in_dtype = _arrays.numpy_dtype_of(D)
    if in_dtype.kind != "c":
        raise ParameterError(f"stft_matrix with dtype={in_dtype} is not of complex type")
    out_dtype = np.dtype(util.dtype_c2r(in_dtype)) if dtype is None else np.dtype(dtype)
    real = np.dtype(np.float64) if (in_dtype == np.complex128 or out_dtype == np.float64) else np.dtype(np.float32)
    cplx = np.dtype(util.dtype_r2c(real))
    n_total = int(D.shape[-1])
    n_frames, n_used, expected = _istft_frame_counts(n_total, n_fft, int(hop_length), bool(center), length)
    lead = tuple(D.shape[:-2])
    shape = lead + (int(expected),)
    if out is not None:
        if is_torch_tensor(D):
            raise ParameterError("out= is only supported for numpy inputs")
        if not np.allclose(out.shape, shape):
            raise ParameterError(f"Shape mismatch for provided output array out.shape={out.shape} != {list(shape)}")
    # window sum-square on the host, in the output precision, exactly as the reference (:606-620)
    wss, wss_key = _istft_wss(window, n_frames, win_length, n_fft, int(hop_length), center, expected, out_dtype, real)
    n_bins = 1 + n_fft // 2
    sess = _arrays.Session(D)
    try:
        ctx = sess.ctx
        plan = ctx.istft_plan(n_fft, int(hop_length), ifft_window.astype(real), bool(center), real)
        batch = int(np.prod(lead, dtype=np.int64)) if lead else 1
        # bring the spectrum into the device layout [batch][frame][bin]
        Dt = _arrays.swap_last_two(D)  # (..., T, bins)
        d_batch_stride, d_frame_stride = n_total * n_bins, n_bins
        if sess.is_torch:
            strides = _frame_major_strides(Dt, n_bins) if Dt.dtype == _arrays.torch_dtype(cplx) else None
            if strides is not None:  # what stft returns (rows possibly padded, see row_pitch), or any frame-major view: read in place
                d_ptr = Dt.data_ptr()
                d_batch_stride, d_frame_stride = strides
                sess._keep.append(Dt)
            else:
                src = D.to(_arrays.torch_dtype(cplx)).contiguous()
                sess._keep.append(src)
                d_ptr = sess.scratch(batch * n_total * n_bins * cplx.itemsize)
                _transpose_batched(ctx, src.data_ptr(), d_ptr, batch, n_bins, n_total, cplx.itemsize)
        else:
            if Dt.flags["C_CONTIGUOUS"] and Dt.dtype == cplx:
                # NumPy in, NumPy out with the spectrum already frame-major (what stft returns): the native host pipeline
                yh = out if (out is not None and out.dtype == real and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]) else np.empty((batch, int(expected)), dtype=real)
                win = ifft_window.astype(real)
                d_item = n_total * n_bins * cplx.itemsize

                def run(c, b, e):
                    pl = plan if c is ctx else c.istft_plan(n_fft, int(hop_length), win, bool(center), real)
                    c.istft_exec_host(pl, Dt.ctypes.data + b * d_item, e - b, n_total, n_used, wss.ctypes.data, yh.ctypes.data + b * int(expected) * real.itemsize, int(expected), int(expected))
                    return False

                ishards = _istft_sample_shards(int(expected), n_used, batch, Dt.nbytes + yh.nbytes, n_fft, int(hop_length), bool(center))
                if ishards is not None:
                    # ONE long spectrogram, fewer clips than devices: device i rebuilds OUTPUT samples shard_range(expected, i, n) from every frame that
                    # reaches into them (its own and the n_fft / hop - 1 on either side), as an uncentred inverse of that run of frames with the matching
                    # piece of the window sum-square envelope; contributions still add in increasing frame order (core/spectrum.py:593-603, 629-643)
                    drop = n_fft // 2 if center else 0

                    def run_samples(c, sh):
                        s0, s1, fa, fb = sh
                        m = n_fft + int(hop_length) * (fb - fa - 1)
                        pl = c.istft_plan(n_fft, int(hop_length), win, False, real)
                        first = fa * int(hop_length) - drop  # final-output coordinate of the shard's first rebuilt sample
                        w_sh = np.ones(m, dtype=real)
                        lo, hi = max(first, 0), min(first + m, int(expected))
                        w_sh[lo - first : hi - first] = wss[lo:hi]
                        part = np.empty((batch, m), dtype=real)
                        for b in range(batch):
                            # one item at a time, its run of frames only: an item of n_total frames taken from frame fa on would end fa frames past the spectrogram
                            c.istft_exec_host(pl, Dt.ctypes.data + (b * n_total + fa) * n_bins * cplx.itemsize, 1, fb - fa, fb - fa, w_sh.ctypes.data,
                                              part.ctypes.data + b * m * real.itemsize, m, m)
                        reach = min(s1, first + m)  # (`length` beyond the last frame's end: zeros there, core/spectrum.py:553-555)
                        yh[:, s0:reach] = part[:, s0 - first : reach - first]
                        yh[:, reach:s1] = 0
                        return False

                    _frame_sharded_host_exec(sess, ishards, run_samples)
                else:
                    _sharded_host_exec(sess, batch, Dt.nbytes + yh.nbytes, run)
                if yh is out:
                    return out
                y = _arrays.cast(yh.reshape(shape), out_dtype)
                if out is not None:
                    out[...] = y
                    return out
                return y
            if Dt.flags["C_CONTIGUOUS"]:
                d_ptr = sess.input_raw(Dt, cplx)
            else:
                src_ptr = sess.input_raw(np.ascontiguousarray(D, dtype=cplx), cplx)
                d_ptr = sess.scratch(batch * n_total * n_bins * cplx.itemsize)
                _transpose_batched(ctx, src_ptr, d_ptr, batch, n_bins, n_total, cplx.itemsize)
        norm_ptr = _device_norm(sess, wss, wss_key, real)
        y_ptr, handle = sess.output((batch, int(expected)), real, rows="flat")
        ctx.istft_exec_norm(plan, d_ptr, batch, d_batch_stride, d_frame_stride, n_used, norm_ptr, y_ptr, int(expected), int(expected))
        y = sess.result(handle)
    finally:
        sess.close()
    y = _arrays.cast(y.reshape(shape), out_dtype)
    if out is not None:
        out[...] = y
        return out
    return y


def _fit_bins(D, n_bins):
    """Crop or zero-pad axis -2 to ``n_bins`` (what ``irfft(..., n=n_fft, axis=-2)`` does to its input)."""
    have = D.shape[-2]
    if have > n_bins:
        return D[..., :n_bins, :]
    if is_torch_tensor(D):
        return _arrays._torch().nn.functional.pad(D, (0, 0, 0, n_bins - have))
    widths = [(0, 0)] * D.ndim
    widths[-2] = (0, n_bins - have)
    return np.pad(D, widths)


def _as_like(sess, host_array):
    if sess.is_torch:
        a = np.ascontiguousarray(host_array)
        if not a.flags.writeable:   # e.g. a broadcast view: torch refuses to wrap read-only memory silently
            a = a.copy()
        return _arrays._torch().from_numpy(a).to(sess.device)
    return host_array


def _transpose_batched(ctx, src_ptr, dst_ptr, batch, rows, cols, elem_bytes):
    """dst[b][c][r] = src[b][r][c]; the native call takes at most 65535 batches per launch."""
    step = 65535
    for b0 in range(0, batch, step):
        nb = min(step, batch - b0)
        off = b0 * rows * cols * elem_bytes
        ctx.transpose(src_ptr + off, dst_ptr + off, nb, rows, cols, elem_bytes)


# ---------------------------------------------------------------------------------------------------
# Griffin-Lim: librosa/core/spectrum.py:2669-2917
# ---------------------------------------------------------------------------------------------------
# griffinlim(init="random") with NumPy's default generator: draw on the device (lra_rng.h) instead of on the host; False = always draw on the host
DEVICE_RNG = True


class _Deprecated:
    """Sentinel for the reference's deprecated ``random_state`` keyword (``util/deprecation.py``)."""

    def __repr__(self):
        return "<DEPRECATED parameter>"


_DEPRECATED = _Deprecated()


def _to_frame_major(sess, x, batch, rows, cols, dtype):
    """(..., rows, cols) array/tensor -> device pointer of its [batch][cols][rows] transpose in ``dtype``."""
    dtype = np.dtype(dtype)
    if sess.is_torch:
        xt = _arrays.swap_last_two(x)
        if xt.dtype == _arrays.torch_dtype(dtype) and (xt.is_contiguous() or (xt.ndim >= 2 and xt.stride(-1) == 1 and xt.stride(-2) >= xt.shape[-1])):
            # frame-major already: in place, or -- rows padded behind the view (stft's device result, row_pitch) -- one compaction pass
            xt = xt.contiguous()
            sess._keep.append(xt)
            return xt.data_ptr()
        src = x.to(_arrays.torch_dtype(dtype)).contiguous()
        sess._keep.append(src)
        src_ptr = src.data_ptr()
    else:
        src_ptr = sess.input_raw(np.ascontiguousarray(x, dtype=dtype), dtype)
    dst = sess.scratch(batch * rows * cols * dtype.itemsize)
    _transpose_batched(sess.ctx, src_ptr, dst, batch, rows, cols, dtype.itemsize)
    return dst


def griffinlim(S, *, n_iter=32, hop_length=None, win_length=None, n_fft=None, window="hann", center=True, dtype=None, length=None, pad_mode="constant",
               momentum=0.99, init="random", rng=None, random_state=_DEPRECATED):
    """"Fast" Griffin-Lim magnitude inversion; drop-in for ``librosa.griffinlim`` (``librosa/core/spectrum.py:2669-2917``).

    The whole fixed-point iteration -- ``istft`` (:2850), ``stft`` (:2863), the phase update with momentum (:2875-2880) --
    runs on the device: the phase estimate, the two rebuilt spectra and the signal stay in HBM for all ``n_iter``
    rounds and only ``S`` (and the host-drawn initial phases, so that ``rng`` reproduces the reference's stream) go up
    and the final signal comes down.  ``S`` may be a device tensor; a device tensor is then returned.

    Differences from the reference: the loop always runs in the precision of ``S`` (``dtype`` is honoured by the final
    ``istft`` only), and ``util.valid_audio`` is checked once after the loop instead of inside every ``stft``.
    """
    if random_state is not _DEPRECATED:
        if rng is not None:
            raise ParameterError(f"Both random_state={random_state!r} and rng={rng!r} were provided. Please use only the rng parameter.")
        warnings.warn("griffinlim() keyword argument 'random_state' has been renamed to 'rng' in version 1.0.0.\n\tThis alias will be removed in version 1.2.0.",
                      category=FutureWarning, stacklevel=2)
        rng = random_state
    if not isinstance(rng, np.random.RandomState):
        rng = np.random.default_rng(rng)
    if momentum > 1:
        warnings.warn(f"Griffin-Lim with momentum={momentum} > 1 can be unstable. Proceed with caution!", stacklevel=2)
    elif momentum < 0:
        raise ParameterError(f"griffinlim() called with momentum={momentum} < 0")
    if init not in ("random", None):
        raise ParameterError(f"init={init} must either None or 'random'")
    if S.ndim < 2:
        raise ParameterError(f"S must have at least 2 dimensions, given shape={tuple(S.shape)}")
    if n_fft is None:
        n_fft = 2 * (S.shape[-2] - 1)
    n_bins, n_total = int(S.shape[-2]), int(S.shape[-1])
    if n_bins != 1 + n_fft // 2:
        # the reference fails at ``angles[:] = rebuilt`` (:2875) with a broadcasting error
        raise ParameterError(f"S has {n_bins} frequency bins, which does not match n_fft={n_fft}")
    if win_length is None:
        win_length = n_fft
    if hop_length is None:
        hop_length = int(win_length // 4)
    elif not util.is_positive_int(hop_length):
        raise ParameterError(f"hop_length={hop_length} must be a positive integer")
    hop = int(hop_length)
    center = bool(center)
    if center and not (isinstance(pad_mode, str) and pad_mode in _DEVICE_PAD_MODES):
        raise ParameterError(f"pad_mode={pad_mode!r} is not supported by librosa_amd.griffinlim")
    s_dtype = _arrays.numpy_dtype_of(S)
    cplx = np.dtype(util.dtype_r2c(s_dtype))
    real = np.dtype(np.float64) if cplx == np.complex128 else np.dtype(np.float32)
    out_dtype = np.dtype(util.dtype_c2r(cplx)) if dtype is None else np.dtype(dtype)
    eps = float(util.tiny(np.empty(0, dtype=cplx)))
    fft_window = util.pad_center(np.asarray(filters.get_window(window, win_length, fftbins=True), dtype=np.float64), size=n_fft)
    n_frames, n_used, expected = _istft_frame_counts(n_total, n_fft, hop, center, length)
    expected = int(expected)
    if not center and n_fft > expected:
        raise ParameterError(f"n_fft={n_fft} is too large for uncentered analysis of input signal of length={expected}")
    rebuilt_frames = 1 + (expected + (2 * (n_fft // 2) if center else 0) - n_fft) // hop
    if rebuilt_frames != n_total:
        raise ParameterError(f"the signal of length {expected} rebuilt from S has {rebuilt_frames} frames, S has {n_total}: could not iterate")
    wss, wss_key = _istft_wss(window, n_frames, win_length, n_fft, hop, center, expected, out_dtype, real)
    lead = tuple(S.shape[:-2])
    batch = int(np.prod(lead, dtype=np.int64)) if lead else 1
    # the uniform draws come from the host generator in the reference's order (S.shape, C order, :2834) so that a seed
    # reproduces its stream; the float64 phasor itself is evaluated on the device
    # ... unless the generator is NumPy's default one (PCG64: default_rng(seed), or rng=None): its stream is reproduced bit for bit on the device
    # (csrc/lra_rng.h) from the generator's state, and the host generator is advanced past the draws -- 92 ms of host work for 32 clips otherwise
    # The caller's generator moves only once the device has taken the draws: a failure before that (plan, frame count, native error) leaves it
    # untouched, and `advance` -- which also drops the generator's cached 32-bit half, something the reference's rng.random() never does -- is followed by
    # putting that half back.
    pcg = None
    n_draws = int(np.prod(S.shape, dtype=np.int64))
    sess = _arrays.Session(S)
    if init == "random" and isinstance(rng, np.random.Generator) and DEVICE_RNG and hasattr(sess.ctx.lib, "lra_griffinlim_init_pcg64"):
        st = rng.bit_generator.state
        if st.get("bit_generator") == "PCG64" and n_draws > 0:
            pcg = (int(st["state"]["state"]), int(st["state"]["inc"]), st.get("has_uint32", 0), st.get("uinteger", 0))
    draws = rng.random(size=tuple(S.shape)) if (init == "random" and pcg is None) else None
    try:
        ctx = sess.ctx
        iplan = ctx.istft_plan(n_fft, hop, fft_window.astype(real), center, real)
        splan = ctx.stft_plan(n_fft, hop, fft_window.astype(real), center, pad_mode if center else "constant", real)
        if ctx.stft_num_frames(splan, expected) != n_total:
            raise ParameterError("internal frame-count mismatch")
        count = batch * n_total * n_bins
        s_ptr = _to_frame_major(sess, S, batch, n_bins, n_total, real)
        angles = sess.scratch(count * cplx.itemsize)
        rebuilt = sess.scratch(count * cplx.itemsize)
        tprev = sess.scratch(count * cplx.itemsize)
        norm_ptr = _device_norm(sess, wss, wss_key, real)
        y_ptr, handle = sess.output((batch, expected), real)
        coef = momentum / (1 + momentum)
        check = ctx.stft_is_fused(splan) and _finite_check_covers_input(expected, n_fft, hop, center)
        if check:
            ctx.nonfinite_reset()
        # angles = S exp(2 pi i u)  (:2834, :2847); the draws travel in S's layout and are transposed on the device.
        # init=None is u = 0: angles = S (1 + 0i)  (:2837)
        if pcg is not None:
            ctx.griffinlim_init_pcg64(pcg[0], pcg[1], s_ptr, angles, batch, n_bins, n_total, real)
            rng.bit_generator.advance(n_draws)  # the generator ends where the reference's rng.random(size=S.shape) leaves it
            st = rng.bit_generator.state
            st["has_uint32"], st["uinteger"] = pcg[2], pcg[3]
            rng.bit_generator.state = st
        else:
            u_t = sess.scratch(count * 8)
            if draws is not None:
                up = sess.input_raw(_as_like(sess, draws.reshape(batch, n_bins, n_total)), np.float64)
                _transpose_batched(ctx, up, u_t, batch, n_bins, n_total, 8)
            else:
                ctx.memset(u_t, 0, count * 8)
            ctx.griffinlim_init(u_t, s_ptr, angles, count, real)
        have_prev = False
        for _ in range(int(n_iter)):
            ctx.istft_exec_norm(iplan, angles, batch, n_total * n_bins, n_bins, n_used, norm_ptr, y_ptr, expected, expected)   # :2850
            ctx.stft_exec(splan, y_ptr, batch, expected, expected, rebuilt)                                                # :2863
            ctx.griffinlim_update(rebuilt, tprev if have_prev else None, s_ptr, angles, count, real, coef, eps)            # :2875-2880
            rebuilt, tprev = tprev, rebuilt                                                                                # :2882
            have_prev = True
        ctx.istft_exec_norm(iplan, angles, batch, n_total * n_bins, n_bins, n_used, norm_ptr, y_ptr, expected, expected)       # :2885
        if check and ctx.nonfinite_read():
            raise ParameterError("Audio buffer is not finite everywhere")
        y = sess.result(handle)
    finally:
        sess.close()
    return _arrays.cast(y.reshape(lead + (expected,)), out_dtype)


# ---------------------------------------------------------------------------------------------------
# phase vocoder: librosa/core/spectrum.py:1364-1519
# ---------------------------------------------------------------------------------------------------
def magphase(D, *, power=1):
    """Separate a spectrogram into magnitude and phase; drop-in for ``librosa.magphase`` (``librosa/core/spectrum.py:1296-1361``):
    ``S = |D| ** power``, ``P = D / |D|`` with ``1 + 0j`` where ``|D| = 0`` (real and imaginary parts divided separately, as the reference does
    for the sake of denormals), so that ``D = S * P`` for ``power = 1``.  ``D``: complex or real, a NumPy array or a device tensor (returned in
    kind), any shape; one elementwise launch (``lra_magphase_exec``)."""
    on_device = is_torch_tensor(D)
    if not on_device:
        D = np.asarray(D)
    in_dtype = _arrays.numpy_dtype_of(D)
    is_complex = in_dtype.kind == "c"
    wide = in_dtype in (np.dtype(np.complex128), np.dtype(np.float64))
    real = np.dtype(np.float64) if wide else np.dtype(np.float32)
    cplx = np.dtype(np.complex128) if wide else np.dtype(np.complex64)
    shape = tuple(int(v) for v in D.shape)
    count = int(np.prod(shape, dtype=np.int64)) if shape else 1
    if count == 0:
        mag, phase = np.zeros(shape, dtype=real), np.zeros(shape, dtype=cplx)
        if on_device:
            torch = _arrays._torch()
            return torch.from_numpy(mag).to(D.device), torch.from_numpy(phase).to(D.device)
        return mag, phase
    sess = _arrays.Session(D if on_device else np.empty(0))
    try:
        ctx = sess.ctx
        if on_device:
            d_ptr = sess.input_raw(D.reshape(-1), cplx if is_complex else real)
        else:
            d_ptr = sess.input_raw(np.ascontiguousarray(D, dtype=cplx if is_complex else real).reshape(-1), cplx if is_complex else real)
        m_ptr, m_handle = sess.output((count,), real)
        p_ptr, p_handle = sess.output((count,), cplx)
        ctx.magphase_exec(d_ptr, is_complex, m_ptr, p_ptr, count, float(power), real)
        mag, phase = sess.result(m_handle), sess.result(p_handle)
    finally:
        sess.close()
    return mag.reshape(shape), phase.reshape(shape)


def phase_vocoder(D, *, rate=None, t_out=None, kind="linear", hop_length=_DEPRECATED, n_fft=_DEPRECATED):
    """Phase vocoder; drop-in for ``librosa.phase_vocoder`` (``librosa/core/spectrum.py:1364-1519``).

    One device kernel: a thread per (clip, bin) accumulates the phase along the output frames and interpolates the
    magnitude (``csrc/lra_post.h``).  ``D`` may be a device tensor (a device tensor is returned).  Only
    ``kind="linear"`` (the default) is provided.
    """
    if D.ndim < 2:
        raise ParameterError(f"D must have at least 2 dimensions, given shape={tuple(D.shape)}")
    n_frames = int(D.shape[-1])
    for name, val in (("hop_length", hop_length), ("n_fft", n_fft)):
        if val is not _DEPRECATED:
            warnings.warn(f"The `{name}` parameter is deprecated as of 1.0 and will be removed in 1.1. It is unused in the current implementation.", FutureWarning, stacklevel=2)
    if (rate is None) == (t_out is None):
        raise ParameterError("Must specify exactly one of `rate` or `t_out`")
    if (rate is not None) and (rate <= 0):
        raise ParameterError(f"rate={rate} must be a positive number")
    if kind != "linear":
        raise ParameterError(f"kind={kind!r}: librosa_amd.phase_vocoder provides linear magnitude interpolation only")
    if t_out is None:
        t_out = np.arange(0.0, n_frames, rate)
    t_out = np.asarray(t_out, dtype=float)
    if np.any(t_out < 0) or np.any(t_out >= n_frames):
        raise ParameterError("t_out values must be in the range [0, D.shape[-1])")
    if np.any(np.diff(t_out) < 0):
        warnings.warn("t_out is not monotonic; phase estimation may be unstable", stacklevel=2)
    in_dtype = _arrays.numpy_dtype_of(D)
    if in_dtype.kind != "c":
        raise ParameterError(f"D with dtype={in_dtype} is not of complex type")
    cplx = np.dtype(in_dtype)
    real = np.dtype(np.float64) if cplx == np.complex128 else np.dtype(np.float32)
    n_bins, n_out = int(D.shape[-2]), int(len(t_out))
    lead = tuple(D.shape[:-2])
    batch = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if n_frames < 2:
        raise ParameterError("phase_vocoder needs at least two frames")
    sess = _arrays.Session(D)
    try:
        ctx = sess.ctx
        d_ptr = _to_frame_major(sess, D, batch, n_bins, n_frames, cplx)
        ptr, handle = sess.output((batch, n_out, n_bins), cplx)
        ctx.phase_vocoder_exec(d_ptr, ptr, batch, n_frames, n_bins, t_out, real)
        res = sess.result(handle)
    finally:
        sess.close()
    return _arrays.swap_last_two(res.reshape(lead + (n_out, n_bins)))


# ---------------------------------------------------------------------------------------------------
# PCEN (the consumer of the streaming STFT, docs/examples/plot_pcen_stream.py:71-80): librosa/core/spectrum.py:2396-2666
# ---------------------------------------------------------------------------------------------------
def pcen(S, *, sr=22050, hop_length=512, gain=0.98, bias=2, power=0.5, time_constant=0.400, eps=1e-6, b=None, max_size=1, ref=None, axis=-1, max_axis=None,
         zi=None, return_zf=False):
    """Per-channel energy normalisation; drop-in for ``librosa.pcen`` (``librosa/core/spectrum.py:2396-2666``).

    ``P = (S / (eps + M)**gain + bias)**power - bias**power`` with ``M`` the first-order IIR smoothing of ``S`` (or of its
    max-filtered version / of ``ref``) along ``axis``, evaluated in the reference's own log-domain form and, like the
    reference, in float64 whatever ``S`` is.  Two device kernels (``csrc/lra_post.h``): the optional band max-filter and one
    fused pass (smoother recurrence per row with the filter state in a register + the elementwise normalisation).  ``zi`` /
    ``return_zf`` carry the filter state between blocks, so ``stream`` -> ``stft(center=False, out=D)`` -> ``pcen(zi=...)``
    runs block by block.  Accepts NumPy arrays or device tensors (device tensors are returned for device input).
    """
    if power < 0:
        raise ParameterError(f"power={power} must be nonnegative")
    if gain < 0:
        raise ParameterError(f"gain={gain} must be non-negative")
    if bias < 0:
        raise ParameterError(f"bias={bias} must be non-negative")
    if eps <= 0:
        raise ParameterError(f"eps={eps} must be strictly positive")
    if time_constant <= 0:
        raise ParameterError(f"time_constant={time_constant} must be strictly positive")
    if not util.is_positive_int(max_size):
        raise ParameterError(f"max_size={max_size} must be a positive integer")
    if b is None:
        t_frames = time_constant * sr / float(hop_length)
        b = (np.sqrt(1 + 4 * t_frames**2) - 1) / (2 * t_frames**2)
    if not 0 <= b <= 1:
        raise ParameterError(f"b={b} must be between 0 and 1")

    on_device = is_torch_tensor(S)
    if not on_device:
        S = np.asarray(S)
    in_dtype = _arrays.numpy_dtype_of(S)
    if in_dtype.kind == "c":
        warnings.warn("pcen was called on complex input so phase information will be discarded. To suppress this warning, call pcen(np.abs(D)) instead.", stacklevel=2)
        S = S.abs() if on_device else np.abs(S)
        in_dtype = _arrays.numpy_dtype_of(S)
    ndim = S.ndim
    if ndim == 0:
        raise ParameterError("pcen needs at least a 1-dimensional input")
    if ref is None and max_size > 1:
        if ndim == 1:
            raise ParameterError("Max-filtering cannot be applied to 1-dimensional input")
        if max_axis is None:
            if ndim != 2:
                raise ParameterError(f"Max-filtering a {ndim:d}-dimensional spectrogram requires you to specify max_axis")
            max_axis = int(np.mod(1 - axis, 2))
    axis = int(axis) % ndim
    shape = tuple(int(n) for n in S.shape)
    if ref is not None:
        if not (is_torch_tensor(ref) or on_device):
            ref = np.asarray(ref)
        if tuple(ref.shape) != shape:
            try:
                ref = ref.expand(shape) if is_torch_tensor(ref) else np.broadcast_to(ref, shape)
            except (RuntimeError, ValueError) as exc:
                raise ParameterError(f"ref of shape {tuple(ref.shape)} does not broadcast to S of shape {shape}") from exc
    # float32 stays float32 on the way in (the kernel widens it); anything else (integers, float64, float16) enters as float64, as NumPy promotes it
    f32_in = in_dtype == np.float32 and (ref is None or _arrays.numpy_dtype_of(ref) == np.float32)
    real = np.dtype(np.float32) if f32_in else np.dtype(np.float64)
    perm = [a for a in range(ndim) if a != axis] + [axis]
    moved = perm != list(range(ndim))
    shape_p = tuple(shape[a] for a in perm)
    n_frames = shape_p[-1]
    rows = int(np.prod(shape_p[:-1], dtype=np.int64)) if ndim > 1 else 1
    state_shape = tuple(1 if a == axis else shape[a] for a in range(ndim))

    def time_last(x):
        if not moved:
            return x
        return x.permute(*perm) if is_torch_tensor(x) else np.transpose(x, perm)

    def time_back(x, shp):
        x = x.reshape(shp)
        if not moved:
            return x
        inv = [int(i) for i in np.argsort(perm)]
        return x.permute(*inv) if is_torch_tensor(x) else np.transpose(x, inv)

    sess = _arrays.Session(S if on_device else np.empty(0))
    try:
        ctx = sess.ctx

        def put(x, dtype):
            if sess.is_torch and not is_torch_tensor(x):
                x = _as_like(sess, np.ascontiguousarray(x))
            return sess.input_raw(x, dtype)

        s_ptr = put(time_last(S), real)
        ref_ptr = None
        if ref is not None:
            ref_ptr = put(time_last(ref), real)
        elif max_size > 1:
            band = perm.index(int(max_axis) % ndim)
            outer = int(np.prod(shape_p[:band], dtype=np.int64))
            inner = int(np.prod(shape_p[band + 1:], dtype=np.int64))
            ref_ptr = sess.scratch(max(rows * n_frames, 1) * real.itemsize)
            ctx.maxfilter_exec(s_ptr, ref_ptr, outer, shape_p[band], inner, int(max_size), real)
        zi_ptr, zi_scalar = None, 0.0
        if zi is None:
            import scipy.signal

            zi_scalar = float(scipy.signal.lfilter_zi([b], [1, b - 1])[0])
        else:
            if not is_torch_tensor(zi):
                zi = np.asarray(zi, dtype=np.float64)
            try:
                zi = zi.expand(state_shape) if is_torch_tensor(zi) else np.broadcast_to(zi, state_shape)
            except (RuntimeError, ValueError) as exc:
                raise ParameterError(f"zi of shape {tuple(zi.shape)} does not match the filter state shape {state_shape}") from exc
            zi_ptr = put(time_last(zi).reshape(-1), np.float64)
        out_ptr, out_handle = sess.output(shape_p, np.float64)
        zf_ptr, zf_handle = sess.output((rows,), np.float64) if return_zf else (None, None)
        ctx.pcen_exec(s_ptr, ref_ptr, out_ptr, rows, n_frames, real, b, gain, bias, power, eps, zi_ptr, zi_scalar, zf_ptr)
        out = time_back(sess.result(out_handle), shape_p)
        zf = time_back(sess.result(zf_handle), shape_p[:-1] + (1,)) if return_zf else None
    finally:
        sess.close()
    return (out, zf) if return_zf else out


# ---------------------------------------------------------------------------------------------------
# decibel scaling: librosa/core/spectrum.py:1735-1883, 1898-1925, 1946-2038, 2054-2082
# ---------------------------------------------------------------------------------------------------
def _db_axes(ndim, axes):
    """``axes="auto"`` -> the last two axes (``core/spectrum.py:1853-1859``); returns a sorted tuple of non-negative axes (empty: reduce nothing ... of a 0-d input)."""
    if isinstance(axes, str):
        if axes != "auto":
            raise ParameterError(f"axes={axes!r} must be 'auto', None, an int or a tuple of ints")
        axes = (-2, -1) if ndim >= 2 else ((-1,) if ndim == 1 else None)
    if axes is None:
        return tuple(range(ndim))
    if isinstance(axes, (int, np.integer)):
        axes = (int(axes),)
    out = sorted({int(a) % ndim for a in axes}) if ndim else []
    return tuple(out)


def _as_items(x, red_axes):
    """Move the reduced axes last and flatten: (array of shape (batch, per_item), restore) with restore(flat) -> original layout."""
    ndim = x.ndim
    keep = [a for a in range(ndim) if a not in red_axes]
    perm = keep + list(red_axes)
    moved = perm != list(range(ndim))
    xp = (x.permute(*perm) if is_torch_tensor(x) else np.transpose(x, perm)) if moved else x
    shape_p = tuple(xp.shape)
    batch = int(np.prod([shape_p[i] for i in range(len(keep))], dtype=np.int64)) if keep else 1
    per_item = int(np.prod(shape_p[len(keep):], dtype=np.int64)) if red_axes else 1

    def restore(flat):
        r = flat.reshape(shape_p)
        if moved:
            inv = np.argsort(perm)
            r = r.permute(*[int(i) for i in inv]) if is_torch_tensor(r) else np.transpose(r, inv)
        return r

    return xp, batch, per_item, restore


def _magnitude_and_dtype(S, name, stacklevel=3):
    """abs() of complex input with the reference's warning (attributed to the caller of the public function: ``stacklevel`` counts from
    here); the real dtype the device computes in (f32 stays f32, everything else f64)."""
    if is_torch_tensor(S):
        if S.is_complex():
            warnings.warn(f"{name} was called on complex input so phase information will be discarded. To suppress this warning, "
                          f"call {name}(np.abs(D){'**2' if name == 'power_to_db' else ''}) instead.", stacklevel=stacklevel)
            S = S.abs()
        real = np.dtype(np.float32) if _arrays.numpy_dtype_of(S) == np.float32 else np.dtype(np.float64)
        return S, real
    S = np.asarray(S)
    if np.issubdtype(S.dtype, np.complexfloating):
        warnings.warn(f"{name} was called on complex input so phase information will be discarded. To suppress this warning, "
                      f"call {name}(np.abs(D){'**2' if name == 'power_to_db' else ''}) instead.", stacklevel=stacklevel)
        S = np.abs(S)
    real = np.dtype(np.float32) if S.dtype == np.float32 else np.dtype(np.float64)
    return S, real


_MAX_CALLABLES = (np.max, np.amax)


def _to_db(S, ref, amin, top_db, axes, amplitude, name):
    if amin <= 0:
        raise ParameterError("amin must be strictly positive")
    if top_db is not None and top_db < 0:
        raise ParameterError("top_db must be non-negative")
    if not callable(ref) and ((ref.ndim if is_torch_tensor(ref) else np.ndim(ref)) > 0):
        return _to_db_array_ref(S, ref, amin, top_db, axes, amplitude, name)
    S, real = _magnitude_and_dtype(S, name)
    scalar_in = S.ndim == 0
    red = _db_axes(S.ndim, axes)
    xp, batch, per_item, restore = _as_items(S, red)
    if batch * per_item == 0:
        return restore(xp.to(_arrays.torch_dtype(real)).reshape(batch, per_item) if is_torch_tensor(xp) else np.asarray(xp, dtype=real).reshape(batch, per_item))
    ref_items_host = None
    ref_scalar = 1.0
    device_max_as_ref = False
    if callable(ref):
        if any(ref is f for f in _MAX_CALLABLES):
            device_max_as_ref = True  # the per-item maximum is reduced on the device (the common ref=np.max)
        else:
            # any other reduction runs on the host exactly as the reference calls it (core/spectrum.py:1861-1869); device
            # tensors are copied down for it (a slow path: prefer ref=np.max or a number)
            # (power_to_db hands real input to `ref` as it is, amplitude_to_db its modulus: core/spectrum.py:1855-1869, 2011-2022)
            host = S.detach().cpu().numpy() if is_torch_tensor(S) else S
            if amplitude:
                host = np.abs(host)
            try:
                rv = ref(host, axis=(red if S.ndim else None), keepdims=True)
            except TypeError as exc:
                raise ParameterError("The provided reference function must support 'axis' and 'keepdims' arguments for proper multichannel processing.") from exc
            rv = np.broadcast_to(np.asarray(rv), tuple(1 if a in red else S.shape[a] for a in range(S.ndim)))
            ref_items_host = np.ascontiguousarray(rv, dtype=real).reshape(-1)
    else:
        ref_scalar = float(np.abs(ref))
    sess = _arrays.Session(S if is_torch_tensor(S) else np.empty(0))
    try:
        ctx = sess.ctx
        x_ptr = sess.input_raw(xp.reshape(batch, per_item) if not is_torch_tensor(xp) else xp.reshape(batch, per_item), real)
        out_ptr, handle = sess.output((batch, per_item), real)
        max_ptr = None
        if device_max_as_ref or top_db is not None:
            max_ptr = sess.scratch(batch * real.itemsize)
            ctx.item_max_exec(x_ptr, batch, per_item, real, max_ptr, absolute=amplitude)  # power_to_db: real input stays signed
        ref_ptr = max_ptr if device_max_as_ref else (sess.input_raw(_as_like(sess, ref_items_host), real) if ref_items_host is not None else None)
        ctx.to_db_exec(x_ptr, out_ptr, batch, per_item, real, amplitude, amin * amin if amplitude else amin, ref_scalar, ref_ptr, max_ptr, top_db)
        out = sess.result(handle)
    finally:
        sess.close()
    out = restore(out)
    return out[()] if scalar_in and not is_torch_tensor(out) else out


def _to_db_array_ref(S, ref, amin, top_db, axes, amplitude, name):
    """Array-valued ``ref`` (anything that broadcasts against ``S``, e.g. one reference per channel; ``core/spectrum.py:1867-1875``):
    the scaling runs on the device with ``ref = 1``, the broadcast subtraction and the ``top_db`` floor on the result."""
    if top_db is not None and top_db < 0:
        raise ParameterError("top_db must be non-negative")
    S, _ = _magnitude_and_dtype(S, name, stacklevel=4)  # the complex-input warning, once, attributed to the public function's caller
    base = _to_db(S, 1.0, amin, None, axes, amplitude, name)  # 10 log10(max(A, mag)) - 10 log10(max(A, 1))
    A = amin * amin if amplitude else amin
    red = _db_axes(base.ndim, axes)
    # |ref| (squared for amplitudes) and its logarithm in ref's OWN precision, as the reference evaluates them (:1869-1875)
    rv = np.abs(ref.detach().cpu().numpy() if is_torch_tensor(ref) else np.asarray(ref))
    rv = rv * rv if amplitude else rv
    if is_torch_tensor(base):
        torch = _arrays._torch()
        ref_db = torch.as_tensor(np.asarray(10.0 * np.log10(np.maximum(A, rv)), dtype=np.float64), device=base.device)
        try:
            out = ((base.to(torch.float64) + 10.0 * np.log10(max(A, 1.0))) - ref_db).to(base.dtype)
        except RuntimeError as exc:
            raise ParameterError(f"ref of shape {tuple(rv.shape)} does not broadcast against the input of shape {tuple(base.shape)}") from exc
        if tuple(out.shape) != tuple(base.shape):
            raise ParameterError(f"ref of shape {tuple(rv.shape)} does not broadcast against the input of shape {tuple(base.shape)}")
        if top_db is not None and red:
            out = torch.maximum(out, out.amax(dim=red, keepdim=True) - top_db)
        return out
    out = np.array(base, copy=True)
    try:
        fits = np.broadcast_shapes(out.shape, np.shape(rv)) == out.shape
    except ValueError:
        fits = False
    if not fits:
        raise ParameterError(f"ref of shape {np.shape(rv)} does not broadcast against the input of shape {out.shape}")
    if A > 1.0:  # (otherwise the device pass subtracted log10(1) = 0: nothing to put back, no extra rounding)
        out += 10.0 * np.log10(A)
    out -= 10.0 * np.log10(np.maximum(A, rv))  # in place: the result keeps the input's precision, as the reference's `log_spec -= ...` does
    if top_db is not None:
        out = np.maximum(out, out.max(axis=red if out.ndim else None, keepdims=True) - top_db)
    return out


def power_to_db(S, *, ref=1.0, amin=1e-10, top_db=80.0, axes="auto"):
    """``10 * log10(S / ref)``, numerically stable; drop-in for ``librosa.power_to_db`` (``librosa/core/spectrum.py:1735-1883``).

    ``log_spec = 10 log10(max(amin, S)) - 10 log10(max(amin, ref))`` and, unless ``top_db`` is None,
    ``max(log_spec, log_spec.max(axes) - top_db)``; with ``axes="auto"`` the maximum (and a callable ``ref``) is taken per
    item over the last two axes.  One device reduction (the per-item maximum, shared by ``ref=np.max`` and ``top_db``) and one
    elementwise pass; accepts NumPy arrays (result downloaded) or device tensors."""
    return _to_db(S, ref, amin, top_db, axes, False, "power_to_db")


def amplitude_to_db(S, *, ref=1.0, amin=1e-5, top_db=80.0, axes="auto"):
    """``power_to_db(S**2, ref=ref**2, amin=amin**2, top_db=top_db)`` as the reference defines it (``core/spectrum.py:1946-2038``)."""
    return _to_db(S, ref, amin, top_db, axes, True, "amplitude_to_db")


def _from_db(S_db, ref, amplitude):
    if is_torch_tensor(ref) or np.ndim(ref) > 0:  # array-valued ref: broadcast on the result (core/spectrum.py:1925, 2082)
        p = _from_db(S_db, 1.0, False)
        if is_torch_tensor(p) and not is_torch_tensor(ref):
            ref = _arrays._torch().as_tensor(np.asarray(ref), device=p.device)
        elif not is_torch_tensor(p) and is_torch_tensor(ref):
            ref = ref.detach().cpu().numpy()
        return (ref ** 2 * p) ** 0.5 if amplitude else ref * p
    x = S_db if is_torch_tensor(S_db) else np.asarray(S_db)
    scalar_in = x.ndim == 0
    real = np.dtype(np.float32) if _arrays.numpy_dtype_of(x) == np.float32 else np.dtype(np.float64)
    count = int(np.prod(x.shape, dtype=np.int64)) if x.ndim else 1
    if count == 0:
        return x
    sess = _arrays.Session(x if is_torch_tensor(x) else np.empty(0))
    try:
        x_ptr = sess.input_raw(x.reshape(-1), real)
        out_ptr, handle = sess.output((count,), real)
        sess.ctx.from_db_exec(x_ptr, out_ptr, count, real, amplitude, float(ref))
        out = sess.result(handle)
    finally:
        sess.close()
    out = out.reshape(tuple(x.shape))
    return out[()] if scalar_in and not is_torch_tensor(out) else out


def db_to_power(S_db, *, ref=1.0):
    """``ref * 10**(S_db / 10)``: inverse of ``power_to_db`` (``librosa/core/spectrum.py:1898-1925``)."""
    return _from_db(S_db, ref, False)


def db_to_amplitude(S_db, *, ref=1.0):
    """``db_to_power(S_db, ref=ref**2) ** 0.5`` (``librosa/core/spectrum.py:2054-2082``)."""
    return _from_db(S_db, ref, True)
