"""``piptrack``, ``pitch_tuning``, ``estimate_tuning``, ``yin`` and ``pyin`` with librosa's signatures (``librosa/core/pitch.py:28-931``).

The tracker is a three-point stencil along the bins of a magnitude spectrogram that is already on the device (``csrc/lra_pitch.h``):
``piptrack`` writes the two dense arrays in one launch (zeros included); ``estimate_tuning`` never forms them -- the same kernel emits only
its peaks, a radix select finds the median of their magnitudes, and the peaks at or above it enter a 1 / ``resolution``-bin integer
histogram.  Only that counts row comes back to the host, which takes the argmax and the edge from the same ``np.linspace`` table as the
reference.  With ``y`` given the magnitude STFT runs first and the spectrogram is never downloaded.

``S`` may be a NumPy array or a device tensor, real or complex (a complex ``S`` goes through the magnitude kernel first; a real one has
``|.|`` taken on load); a device tensor in the layout ``stft`` / ``_spectrogram`` return is read in place.  ``S`` is never written.

``ref``: ``None`` / ``np.max`` and numbers are handled in the kernel.  Any other callable is the slow path: it is applied on the host to a
NumPy copy of ``|S|`` and its per-frame row is uploaded.

``yin`` is one launch of ``csrc/lra_yin.h`` that reads the samples once and writes one float64 per frame: the autocorrelation of every frame
through a mixed-radix transform (a direct sum where no compiled size holds ``frame_length + max_period``), the difference function, its
cumulative mean normalisation, the first trough below the threshold and the parabola at that lag.  Everything after the load is float64, for
float32 samples too, and ``f0`` is float64 as the reference's is.  ``_yin_frames`` returns the dense front half that ``pyin`` shares.

Documented difference: ``yin`` with ``frame_length + max_period > 4800`` (no compiled transform) and ``max_period > 10239`` raises
``ParameterError`` before any device work: the direct kernel keeps 16 bytes per lag in a workgroup's 160 KiB of LDS (sr 44100,
``frame_length=16384``, ``fmin=4`` is such a call; the reference accepts it).

``pyin`` runs, per chunk of whole clips sized by ``sequence.SCRATCH_BUDGET``: the same front half on float64 samples (float32 input is widened
first, on the device for a tensor); one launch of ``csrc/lra_pyin.h``'s observation kernel, which turns the CMND and the shifts into the float64
log observation table in the decoder's layout and ``voiced_prob`` -- the thresholds, ``beta_probs``, their prefix sums and the two factors of
SciPy's Boltzmann pmf are host tables built as the reference builds them; ``lra_viterbi_exec`` on that resident table with the reference's
transition and ``p_init`` (``sequence._ResidentDecoder``); and an elementwise lookup of ``f0`` and ``voiced_flag``.

Documented differences of ``pyin``: the reference's float32 cancellation noise is not reproduced (``pyin(y32)`` equals
``pyin(y32.astype(float64))``); ``2 * n_pitch_bins > 8192`` (the default range at ``resolution=0.01``), ``n_thresholds`` that is not a positive
integer, a non-positive ``boltzmann_parameter`` or ``resolution``, and ``8 * (n_pitch_bins + n_thresholds)`` bytes beyond a workgroup's 160 KiB of
LDS raise ``ParameterError`` before any device work, as ``yin``'s refusal below does.

Documented difference: an ``S`` with fewer than two bins raises ``ParameterError`` (the reference fails incidentally there, with
``ZeroDivisionError`` or ``np.gradient``'s ``ValueError``).  ``S`` must be floating-point or complex.
"""
from __future__ import annotations

import warnings

import numpy as np

from .. import _arrays, _native
from ..util.exceptions import ParameterError
from ..util.utils import is_torch_tensor, valid_audio
from . import convert
from . import spectrum as _spectrum

__all__ = ["piptrack", "pitch_tuning", "estimate_tuning", "yin", "pyin"]

_YIN_F0, _YIN_FRAMES = 0, 1  # the LRA_YIN_* values
_YIN_LDS_MAX = 160 * 1024  # LRA_YIN_LDS_MAX
_PIPTRACK_KWARGS = ("hop_length", "fmin", "fmax", "threshold", "win_length", "window", "center", "pad_mode", "ref")


def _is_number(x):
    return isinstance(x, (int, float, np.number)) and not isinstance(x, (bool, np.bool_))


def _bin_range(sr, n_fft, fmin, fmax):
    """The bins of ``freq_mask = (fmin <= fft_freqs) & (fft_freqs < fmax)`` (``core/pitch.py:326-344``, float64) as ``lo <= f < hi``."""
    fmin = np.maximum(fmin, 0)
    fmax = np.minimum(fmax, float(sr) / 2)
    freqs = convert.fft_frequencies(sr=sr, n_fft=n_fft)
    hit = np.flatnonzero((fmin <= freqs) & (freqs < fmax))
    if hit.size == 0:
        return 0, 0
    lo, hi = int(hit[0]), int(hit[-1]) + 1
    if hi - lo != hit.size:
        raise ParameterError(f"the bins between fmin={fmin} and fmax={fmax} are not one range (sr={sr})")
    return lo, hi


def _check_args(sr, threshold, ref, fmin, fmax):
    if not (_is_number(sr) and sr > 0):
        raise ParameterError(f"sr={sr!r} must be a positive number")
    if not _is_number(threshold):
        raise ParameterError(f"threshold={threshold!r} must be a number")
    if not (_is_number(fmin) and _is_number(fmax)):
        raise ParameterError(f"fmin={fmin!r} and fmax={fmax!r} must be numbers")
    if not (ref is None or callable(ref) or _is_number(ref)):
        raise ParameterError(f"ref={ref!r} must be None, a number or a callable")


def _check_S(S):
    dtype = _arrays.numpy_dtype_of(S)
    if dtype not in (np.float32, np.float64, np.complex64, np.complex128):
        raise ParameterError(f"S must be floating-point or complex, given dtype={dtype}")
    if S.ndim < 2:
        raise ParameterError(f"S must have at least 2 dimensions, given shape={tuple(S.shape)}")
    if S.shape[-2] < 2:
        raise ParameterError(f"S must have at least 2 frequency bins, given shape={tuple(S.shape)}")
    return np.dtype(np.float64) if dtype in (np.float64, np.complex128) else np.dtype(np.float32)


def _host_ref_row(S, ref, threshold, lead, n_frames):
    """The slow path of a callable ``ref``: ``threshold * ref(|S|, axis=-2)`` on the host, one float64 value per frame."""
    host = S.detach().cpu().numpy() if is_torch_tensor(S) else np.asarray(S)
    if np.iscomplexobj(host) or (host.size and host.min() < 0):
        host = np.abs(host)
    row = np.asarray(threshold * ref(host, axis=-2))
    if row.ndim == host.ndim:  # (a callable that keeps the reduced axis)
        row = np.squeeze(row, axis=-2)
    return np.ascontiguousarray(np.broadcast_to(row, lead + (n_frames,)), dtype=np.float64)


def _ref_args(sess, S, ref, threshold, lead, n_frames):
    """(mode, threshold, device pointer of the per-frame row, scalar) for the kernels."""
    ctx = sess.ctx
    if ref is None or ref is np.max or ref is np.amax:
        return ctx.PITCH_REF_MAX, float(threshold), 0, 0.0
    if callable(ref):
        row = _host_ref_row(S, ref, threshold, lead, n_frames)
        return ctx.PITCH_REF_ROW, float(threshold), sess.input_raw(_spectrum._as_like(sess, row), np.float64), 0.0
    return ctx.PITCH_REF_SCALAR, float(threshold), 0, float(np.abs(ref))


def _resident(sess, S, real):
    """Device pointer of the real magnitudes of ``S`` (..., n_bins, n_frames), its (batch, bin, frame) strides in elements, and whether that
    is the frame-major form.  A device tensor in the layout of ``stft`` / ``_spectrogram`` is used in place; a complex ``S`` is rectified by
    the magnitude kernel into scratch."""
    n_bins, n_frames = int(S.shape[-2]), int(S.shape[-1])
    dtype = _arrays.numpy_dtype_of(S)
    St = _arrays.swap_last_two(S)  # (..., t, f)
    if is_torch_tensor(S):
        if dtype.kind != "c":
            rows = _spectrum._frame_major_strides(St, n_bins)
            if rows is not None:
                sess._keep.append(St)
                return St.data_ptr(), (rows[0], 1, rows[1]), True
        frame_major = St.is_contiguous()
    else:
        frame_major = bool(St.flags["C_CONTIGUOUS"]) and n_frames > 1  # a view of the device layout (what our own _spectrogram returns)
    src = St if frame_major else S
    strides = (n_frames * n_bins, 1, n_bins) if frame_major else (n_bins * n_frames, n_frames, 1)
    ptr = sess.input_raw(src, dtype)
    if dtype.kind == "c":
        count = int(np.prod(S.shape, dtype=np.int64))
        mag = sess.scratch(count * real.itemsize)
        sess.ctx.magnitude_exec(ptr, mag, count, real)
        ptr = mag
    return ptr, strides, frame_major


def _dense(sess, s_ptr, strides, frame_major, batch, n_bins, n_frames, real, lo, hi, ref_args, sr, n_fft):
    """One launch; returns the handle of the (2, batch, n_frames, n_bins) -- frame-major -- or (2, batch, n_bins, n_frames) result."""
    shape = (2, batch, n_frames, n_bins) if frame_major else (2, batch, n_bins, n_frames)
    out_ptr, handle = sess.output(shape, real)
    out_strides = (n_frames * n_bins, 1, n_bins) if frame_major else (n_bins * n_frames, n_frames, 1)
    mode, threshold, row_ptr, scalar = ref_args
    sess.ctx.piptrack_exec(s_ptr, batch, n_bins, n_frames, strides, real, lo, hi, mode, threshold, row_ptr, scalar, sr, n_fft, out_ptr,
                           out_ptr + batch * n_frames * n_bins * real.itemsize, out_strides)
    return handle


def _split(res, lead, n_bins, n_frames, frame_major):
    if frame_major:
        res = _arrays.swap_last_two(res.reshape((2,) + lead + (n_frames, n_bins)))  # the view convention of stft / _spectrogram
    else:
        res = res.reshape((2,) + lead + (n_bins, n_frames))
    return res[0], res[1]


def piptrack(*, y=None, sr=22050, S=None, n_fft=2048, hop_length=None, fmin=150.0, fmax=4000.0, threshold=0.1, win_length=None, window="hann", center=True, pad_mode="constant",
             ref=None):
    """Pitch tracking on the thresholded, parabolically interpolated magnitude spectrogram; drop-in for ``librosa.piptrack``
    (``core/pitch.py:181-366``).  Returns ``(pitches, magnitudes)``, shaped and typed like ``S`` (a real array of the same precision for a
    complex ``S``), NumPy arrays for NumPy input and device tensors for device tensors, zero everywhere but at the detected peaks.

    With ``y`` the magnitude STFT and the tracker run back to back on the device.  See the module docstring for ``ref`` and the layouts."""
    _check_args(sr, threshold, ref, fmin, fmax)
    if S is None and y is not None and callable(ref) and not (ref is np.max or ref is np.amax):
        S, n_fft = _spectrum._spectrogram(y=y, n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window, center=center, pad_mode=pad_mode)
    if S is not None:
        real = _check_S(S)
        S, n_fft = _spectrum._spectrogram(S=S, n_fft=n_fft)
        lead = tuple(int(s) for s in S.shape[:-2])
        n_bins, n_frames = int(S.shape[-2]), int(S.shape[-1])
        batch = int(np.prod(lead, dtype=np.int64)) if lead else 1
        lo, hi = _bin_range(sr, n_fft, fmin, fmax)
        sess = _arrays.Session(S)
        try:
            if batch * n_frames == 0:
                handle, frame_major = sess.output((2, batch, n_bins, n_frames), real)[1], False
            else:
                ref_args = _ref_args(sess, S, ref, threshold, lead, n_frames)
                s_ptr, strides, frame_major = _resident(sess, S, real)
                handle = _dense(sess, s_ptr, strides, frame_major, batch, n_bins, n_frames, real, lo, hi, ref_args, float(sr), n_fft)
            res = sess.result(handle)
        finally:
            sess.close()
        return _split(res, lead, n_bins, n_frames, frame_major)
    if n_fft is None:
        raise ParameterError(f"Unable to compute spectrogram with n_fft={n_fft}")
    if y is None:
        raise ParameterError("Input signal must be provided to compute a spectrogram")
    lo, hi = _bin_range(sr, n_fft, fmin, fmax)
    shape = {}

    def post(sess, s_ptr, batch, n_bins, n_frames, pitch, real):
        shape.update(n_bins=n_bins, n_frames=n_frames)
        ref_args = _ref_args(sess, None, ref, threshold, (), n_frames)
        return _dense(sess, s_ptr, (n_frames * pitch, 1, pitch), True, batch, n_bins, n_frames, real, lo, hi, ref_args, float(sr), n_fft), None

    res = _spectrum._run_stft_family("power", y, n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window, center=center, pad_mode=pad_mode, power=1.0, post=post)
    return _split(res, tuple(int(s) for s in y.shape[:-1]), shape["n_bins"], shape["n_frames"], True)


def _edges_ptr(sess, edges):
    ctx = sess.ctx
    if ctx.table_cacheable(edges.nbytes):
        return ctx.device_table(("tuning_edges", int(edges.size)), lambda: edges)
    return sess.input_raw(_spectrum._as_like(sess, edges), np.float64)


def _histogram_edges(resolution, bins_per_octave):
    if not (_is_number(resolution) and resolution > 0):
        raise ParameterError(f"resolution={resolution!r} must be a positive number")
    if not (_is_number(bins_per_octave) and bins_per_octave > 0):
        raise ParameterError(f"bins_per_octave={bins_per_octave!r} must be a positive number")
    n_hist = int(np.ceil(1.0 / resolution))
    if n_hist < 1 or n_hist > 2**31 - 3:
        raise ParameterError(f"resolution={resolution!r} gives {n_hist} histogram bins")
    return np.linspace(-0.5, 0.5, n_hist + 1)


def _host_row(row):
    return row.detach().cpu().numpy() if is_torch_tensor(row) else np.asarray(row)


def _tuning_from_counts(row, edges, stacklevel):
    """The histogram's first maximum and its left edge (``core/pitch.py:153-178``); ``row``: the counts, then how many frequencies entered."""
    n_hist = edges.size - 1
    if row is None or int(row[n_hist]) == 0:
        warnings.warn("Trying to estimate tuning from empty frequency set.", stacklevel=stacklevel)
        return 0.0
    return float(edges[int(np.argmax(row[:n_hist]))])


def _pitch_tuning_row(frequencies, resolution, bins_per_octave):
    """``pitch_tuning`` up to the histogram: (the counts row of ``lra_pitch_tuning_exec``, or None for an empty input; the edges)."""
    edges = _histogram_edges(resolution, bins_per_octave)
    if not is_torch_tensor(frequencies):
        frequencies = np.atleast_1d(frequencies)
        if frequencies.dtype.kind not in "fiub":
            raise ParameterError(f"frequencies must be real numbers, given dtype={frequencies.dtype}")
        if frequencies.dtype not in (np.float32, np.float64):
            frequencies = frequencies.astype(np.float64)
    real = _arrays.numpy_dtype_of(frequencies)
    if real not in (np.float32, np.float64):
        raise ParameterError(f"frequencies must be real floating-point, given dtype={real}")
    n = int(np.prod(frequencies.shape, dtype=np.int64))
    if n == 0:
        return None, edges
    sess = _arrays.Session(frequencies)
    try:
        out_ptr, handle = sess.output((edges.size + 1,), np.int64)
        sess.ctx.pitch_tuning_exec(sess.input_raw(frequencies, real), n, real, _edges_ptr(sess, edges), edges.size - 1, bins_per_octave, out_ptr)
        row = sess.result(handle)
    finally:
        sess.close()
    return _host_row(row), edges


def pitch_tuning(frequencies, *, resolution=0.01, bins_per_octave=12):
    """The tuning offset of a collection of frequencies relative to A440, in fractions of a bin; drop-in for ``librosa.pitch_tuning``
    (``core/pitch.py:112-178``).  ``frequencies``: array-like or device tensor.  Returns a Python float."""
    row, edges = _pitch_tuning_row(frequencies, resolution, bins_per_octave)
    return _tuning_from_counts(row, edges, 3)


def _tuning_row(y, sr, S, n_fft, resolution, bins_per_octave, kwargs):
    """``estimate_tuning`` up to the histogram: (the counts row of ``lra_tuning_exec`` as a NumPy array, or None for an empty input; the edges)."""
    unknown = sorted(set(kwargs) - set(_PIPTRACK_KWARGS))
    if unknown:
        raise TypeError(f"piptrack() got an unexpected keyword argument {unknown[0]!r}")
    fmin, fmax, threshold, ref = kwargs.get("fmin", 150.0), kwargs.get("fmax", 4000.0), kwargs.get("threshold", 0.1), kwargs.get("ref", None)
    stft_kwargs = {k: kwargs[k] for k in ("hop_length", "win_length", "window", "center", "pad_mode") if k in kwargs}
    _check_args(sr, threshold, ref, fmin, fmax)
    edges = _histogram_edges(resolution, bins_per_octave)
    if S is None and y is not None and callable(ref) and not (ref is np.max or ref is np.amax):
        S, n_fft = _spectrum._spectrogram(y=y, n_fft=n_fft, **{"hop_length": None, **stft_kwargs})

    def run(sess, s_ptr, strides, batch, n_bins, n_frames, real, lo, hi, ref_args):
        out_ptr, handle = sess.output((edges.size + 1,), np.int64)
        mode, thr, row_ptr, scalar = ref_args
        work = sess.scratch(sess.ctx.tuning_work_bytes(batch, n_frames, hi - lo, real))
        sess.ctx.tuning_exec(s_ptr, batch, n_bins, n_frames, strides, real, lo, hi, mode, thr, row_ptr, scalar, float(sr), n_fft, _edges_ptr(sess, edges), edges.size - 1,
                             bins_per_octave, work, out_ptr)
        return handle

    if S is not None:
        real = _check_S(S)
        S, n_fft = _spectrum._spectrogram(S=S, n_fft=n_fft)
        lead = tuple(int(s) for s in S.shape[:-2])
        n_bins, n_frames = int(S.shape[-2]), int(S.shape[-1])
        batch = int(np.prod(lead, dtype=np.int64)) if lead else 1
        lo, hi = _bin_range(sr, n_fft, fmin, fmax)
        if batch * n_frames == 0:
            return None, edges
        sess = _arrays.Session(S)
        try:
            ref_args = _ref_args(sess, S, ref, threshold, lead, n_frames)
            s_ptr, strides, _ = _resident(sess, S, real)
            row = sess.result(run(sess, s_ptr, strides, batch, n_bins, n_frames, real, lo, hi, ref_args))
        finally:
            sess.close()
        return _host_row(row), edges
    if n_fft is None:
        raise ParameterError(f"Unable to compute spectrogram with n_fft={n_fft}")
    if y is None:
        raise ParameterError("Input signal must be provided to compute a spectrogram")
    lo, hi = _bin_range(sr, n_fft, fmin, fmax)

    def post(sess, s_ptr, batch, n_bins, n_frames, pitch, real):
        ref_args = _ref_args(sess, None, ref, threshold, (), n_frames)
        return run(sess, s_ptr, (n_frames * pitch, 1, pitch), batch, n_bins, n_frames, real, lo, hi, ref_args), None

    row = _spectrum._run_stft_family("power", y, n_fft=n_fft, power=1.0, post=post, **{"hop_length": None, "win_length": None, "window": "hann", "center": True, "pad_mode": "constant", **stft_kwargs})
    return _host_row(row), edges


def estimate_tuning(*, y=None, sr=22050, S=None, n_fft=2048, resolution=0.01, bins_per_octave=12, **kwargs):
    """The tuning of a signal or a spectrogram; drop-in for ``librosa.estimate_tuning`` (``core/pitch.py:28-109``).  ``kwargs`` go to
    ``piptrack``.  All leading dimensions count towards one estimate.  Returns a Python float; the dense ``piptrack`` arrays are never formed
    and only the histogram's counts leave the device, so ``chroma_stft(y=y, sr=sr, tuning=estimate_tuning(y=y, sr=sr))`` stays resident."""
    row, edges = _tuning_row(y, sr, S, n_fft, resolution, bins_per_octave, kwargs)
    return _tuning_from_counts(row, edges, 3)


def _check_yin_params(*, sr, fmax, fmin, frame_length):
    """``__check_yin_params`` (``core/pitch.py:934-968``), with its messages."""
    if fmax > sr / 2:
        raise ParameterError(f"fmax={fmax:.3f} cannot exceed Nyquist frequency {sr/2}")
    if fmin >= fmax:
        raise ParameterError(f"fmin={fmin:.3f} must be less than fmax={fmax:.3f}")
    if fmin <= 0:
        raise ParameterError(f"fmin={fmin:.3f} must be strictly positive")
    if sr / fmin >= frame_length - 1:
        fmin_feasible = sr / (frame_length - 1)
        frame_length_feasible = int(np.ceil(sr / fmin) + 1)
        raise ParameterError(f"fmin={fmin:.3f} is too small for frame_length={frame_length} and sr={sr}. "
                             f"Either increase to fmin={fmin_feasible:.3f} or frame_length={frame_length_feasible}")
    if sr / fmin >= frame_length // 2:
        fmin_optimal = sr / (frame_length / 2)
        frame_length_optimal = int(np.ceil(sr / fmin) * 2 + 1)
        warnings.warn(f"With fmin={fmin:.3f}, sr={sr} and frame_length={frame_length}, less than two periods of fmin "
                      f"fit into the frame, which can cause inaccurate pitch detection. "
                      f"Consider increasing to fmin={fmin_optimal:.3f} or frame_length={frame_length_optimal}.", stacklevel=5)


def _yin_prepare(y, fmin, fmax, sr, frame_length, hop_length, center, pad_mode):
    """Every check of the reference's ``yin`` in its order (``core/pitch.py:562-585``), before any device work.  Returns the samples (padded
    on the host for a pad mode the kernel does not fold into its load), their real type, hop, centre flag, pad mode and both periods."""
    if fmin is None or fmax is None:
        raise ParameterError('both "fmin" and "fmax" must be provided')
    _check_yin_params(sr=sr, fmax=fmax, fmin=fmin, frame_length=frame_length)
    if hop_length is None:
        hop_length = frame_length // 4
    if is_torch_tensor(y):
        _spectrum._validate_audio(y, True)
        if not _spectrum._all_finite(y):
            raise ParameterError("Audio buffer is not finite everywhere")
    else:
        valid_audio(y)
    real = np.dtype(np.float64) if _arrays.numpy_dtype_of(y) == np.float64 else np.dtype(np.float32)
    center = bool(center)
    if center and not (isinstance(pad_mode, str) and pad_mode in _spectrum._DEVICE_PAD_MODES):
        if is_torch_tensor(y):
            raise ParameterError(f"pad_mode={pad_mode!r} is only supported for numpy inputs")
        widths = [(0, 0)] * y.ndim
        widths[-1] = (frame_length // 2, frame_length // 2)
        y = np.pad(y, widths, mode=pad_mode)
        center = False
    if not center:
        pad_mode = "constant"
    n = int(y.shape[-1]) + (2 * (frame_length // 2) if center else 0)
    if n < frame_length:
        raise ParameterError(f"Input is too short (n={n:d}) for frame_length={frame_length:d}")
    if hop_length < 1:
        raise ParameterError(f"Invalid hop_length: {hop_length:d}")
    min_period = int(np.floor(sr / fmax))
    max_period = min(int(np.ceil(sr / fmin)), frame_length - 1)
    if _native.load_library().lra_yin_lds_bytes(int(frame_length), max_period) > _YIN_LDS_MAX:
        # documented difference: no compiled transform holds frame_length + max_period and the direct kernel's two rows of lags outgrow a workgroup's LDS
        raise ParameterError(f"fmin={fmin:.3f} gives max_period={max_period}, too long for frame_length={frame_length} on the device: "
                             f"the direct kernel serves max_period <= {_YIN_LDS_MAX // 16 - 1}")
    return y, real, int(hop_length), center, pad_mode, min_period, max_period


def _yin_run(y, mode, fmin, fmax, sr, frame_length, hop_length, trough_threshold, center, pad_mode):
    y, real, hop, center, pad_mode, min_period, max_period = _yin_prepare(y, fmin, fmax, sr, frame_length, hop_length, center, pad_mode)
    return _yin_launch(y, real, mode, sr, frame_length, hop, trough_threshold, center, pad_mode, min_period, max_period)


def _yin_launch(y, real, mode, sr, frame_length, hop, trough_threshold, center, pad_mode, min_period, max_period):
    """One ``lra_yin_exec`` on samples that ``_yin_prepare`` has passed."""
    lead = tuple(int(s) for s in y.shape[:-1])
    n = int(y.shape[-1])
    batch = int(np.prod(lead, dtype=np.int64)) if lead else 1
    n_frames = 1 + (n + (2 * (frame_length // 2) if center else 0) - frame_length) // hop
    n_lags = max_period - min_period + 1
    sess = _arrays.Session(y)
    try:
        ctx = sess.ctx
        frames = mode == _YIN_FRAMES
        out_ptr, handle = sess.output((2, batch, n_lags, n_frames) if frames else (batch, n_frames), real if frames else np.float64)
        if batch > 0:
            y_ptr = sess.input_2d(y, real)[0]
            half = batch * n_lags * n_frames * real.itemsize
            ctx.yin_exec(y_ptr, batch, n, real, frame_length, hop, center, pad_mode, min_period, max_period, float(trough_threshold), float(sr), mode,
                         f0_ptr=0 if frames else out_ptr, frames_ptr=out_ptr if frames else 0, shifts_ptr=out_ptr + half if frames else 0)
        res = sess.result(handle)
    finally:
        sess.close()
    if frames:
        res = res.reshape((2,) + lead + (n_lags, n_frames))
        return res[0], res[1], min_period
    return res.reshape(lead + (n_frames,))


def yin(y, *, fmin, fmax, sr=22050, frame_length=2048, hop_length=None, trough_threshold=0.1, center=True, pad_mode="constant"):
    """Fundamental frequency estimation with the YIN algorithm; drop-in for ``librosa.yin`` (``core/pitch.py:480-628``).

    ``y``: (..., n) NumPy array or device tensor, float32 or float64.  Returns ``f0`` (..., n_frames) in float64: a NumPy array for NumPy input,
    a device tensor for a device tensor.  ``pad_mode``: "constant", "reflect", "edge" and "symmetric" are folded into the kernel's load; any
    other ``np.pad`` mode is applied on the host, for NumPy input only.  ``y`` is never written."""
    return _yin_run(y, _YIN_F0, fmin, fmax, sr, frame_length, hop_length, trough_threshold, center, pad_mode)


def _yin_frames(y, *, fmin, fmax, sr=22050, frame_length=2048, hop_length=None, center=True, pad_mode="constant"):
    """The front half ``yin`` and ``pyin`` share (``core/pitch.py:583-593``): ``(yin_frames, parabolic_shifts, min_period)`` with the cumulative
    mean normalised difference function and the parabolic shifts as (..., max_period - min_period + 1, n_frames) arrays of ``y``'s type
    (computed in float64 and rounded once)."""
    return _yin_run(y, _YIN_FRAMES, fmin, fmax, sr, frame_length, hop_length, 0.0, center, pad_mode)


def _pyin_tables(n_lags, n_thresholds, beta_parameters, boltzmann_parameter):
    """The host tables of the observation kernel, built as the reference builds them (``core/pitch.py:802-804``, ``:892-894``): thresholds[1:],
    beta_probs, np.sum(beta_probs[:m]) for every m, and the two factors of scipy's ``boltzmann._pmf`` = fact[N] * E[k]."""
    key = (int(n_lags), int(n_thresholds), tuple(float(b) for b in beta_parameters), boltzmann_parameter)
    if key not in _PYIN_TABLES:
        import scipy.stats

        thresholds = np.linspace(0, 1, n_thresholds + 1)
        beta_probs = np.diff(scipy.stats.beta.cdf(thresholds, beta_parameters[0], beta_parameters[1]))
        prefix = np.array([np.sum(beta_probs[:m]) for m in range(n_thresholds + 1)], dtype=np.float64)
        lambda_ = np.asarray(boltzmann_parameter)
        k = np.arange(n_lags + 1)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            e = np.exp(-lambda_ * k).astype(np.float64)
            fact = ((1 - np.exp(-lambda_)) / (1 - np.exp(-lambda_ * k))).astype(np.float64)
        fact[0] = 0.0   # (no trough below the threshold: never read)
        if len(_PYIN_TABLES) >= 8:
            _PYIN_TABLES.clear()
        _PYIN_TABLES[key] = (np.ascontiguousarray(thresholds[1:]), np.ascontiguousarray(beta_probs, dtype=np.float64), prefix, e, fact)
    return _PYIN_TABLES[key]


_PYIN_TABLES = {}
_PYIN_DECODERS = {}
_PYIN_LDS_MAX = 160 * 1024  # LRA_PYIN_LDS_MAX


def _pyin_bins(fmin, fmax, resolution, n_thresholds, boltzmann_parameter):
    """``n_bins_per_semitone`` and ``n_pitch_bins`` (``core/pitch.py:806-807``), and the limits of the device path, before any device work."""
    from .. import sequence as _sequence

    if isinstance(n_thresholds, (bool, np.bool_)) or not isinstance(n_thresholds, (int, np.integer)) or n_thresholds < 1:
        raise ParameterError(f"n_thresholds={n_thresholds!r} must be a positive integer")
    if not (_is_number(boltzmann_parameter) and boltzmann_parameter > 0):
        raise ParameterError(f"boltzmann_parameter={boltzmann_parameter!r} must be a positive number")
    if not (_is_number(resolution) and resolution > 0):
        raise ParameterError(f"resolution={resolution!r} must be a positive number")
    n_bins_per_semitone = int(np.ceil(1.0 / resolution))
    n_pitch_bins = int(np.floor(12 * n_bins_per_semitone * np.log2(fmax / fmin))) + 1
    _sequence._check_states(2 * n_pitch_bins)   # documented difference: the decoder's limit
    if _native.load_library().lra_pyin_lds_bytes(n_pitch_bins, int(n_thresholds)) > _PYIN_LDS_MAX:
        # documented difference: a frame's voiced row and two counters per threshold live in the LDS of one workgroup
        raise ParameterError(f"n_thresholds={n_thresholds} with {n_pitch_bins} pitch bins is too large for the device: 8 bytes per pitch bin and per threshold must fit {_PYIN_LDS_MAX} bytes")
    return n_bins_per_semitone, n_pitch_bins


def _pyin_obs(sess, cm_ptr, sh_ptr, clips, n_lags, n_frames, log_prob_ptr, voiced_ptr, *, sr, fmin, min_period, n_thresholds, beta_parameters, boltzmann_parameter, n_pitch_bins,
              n_bins_per_semitone, no_trough_prob):
    """One launch of the observation kernel on resident float64 CMND and shifts [clip][lag][frame]."""
    from ..util.utils import tiny

    up = lambda a: sess.input_raw(_spectrum._as_like(sess, a), np.float64)
    thresholds, beta_probs, prefix, e, fact = _pyin_tables(n_lags, n_thresholds, beta_parameters, boltzmann_parameter)
    eps = tiny(np.empty(0, dtype=np.float64))
    sess.ctx.pyin_obs_exec(cm_ptr, sh_ptr, clips, n_lags, n_frames, up(thresholds), up(beta_probs), up(prefix), up(e), up(fact), int(n_thresholds), float(sr), float(fmin), int(min_period),
                           n_pitch_bins, n_bins_per_semitone, float(no_trough_prob), float(eps), float(np.log(0.0 + eps)), log_prob_ptr, voiced_ptr)


def _pyin_log_prob(yin_frames, parabolic_shifts, *, sr, fmin, fmax, min_period, n_thresholds=100, beta_parameters=(2, 18), boltzmann_parameter=2, resolution=0.1, no_trough_prob=0.01):
    """The observation stage of ``pyin`` alone (``core/pitch.py:796-825``, ``__pyin_helper``) on arrays as given: ``yin_frames`` and
    ``parabolic_shifts`` of shape (..., n_lags, n_frames).  Returns ``log(observation_probs + tiny)`` (..., 2 * n_pitch_bins, n_frames) -- a view of
    the decoder's own (..., n_frames, 2 * n_pitch_bins) layout -- and ``voiced_prob`` (..., n_frames), float64."""
    n_bins_per_semitone, n_pitch_bins = _pyin_bins(fmin, fmax, resolution, n_thresholds, boltzmann_parameter)
    if tuple(yin_frames.shape) != tuple(parabolic_shifts.shape) or yin_frames.ndim < 2 or yin_frames.shape[-2] < 2:
        raise ParameterError(f"yin_frames.shape={tuple(yin_frames.shape)} and parabolic_shifts.shape={tuple(parabolic_shifts.shape)} must be equal, (..., n_lags >= 2, n_frames)")
    lead = tuple(int(s) for s in yin_frames.shape[:-2])
    n_lags, n_frames = int(yin_frames.shape[-2]), int(yin_frames.shape[-1])
    clips = int(np.prod(lead, dtype=np.int64)) if lead else 1
    sess = _arrays.Session(yin_frames)
    try:
        lp_ptr, lp_h = sess.output((clips, n_frames, 2 * n_pitch_bins), np.float64)
        vp_ptr, vp_h = sess.output((clips, n_frames), np.float64)
        if clips * n_frames > 0:
            _pyin_obs(sess, sess.input_raw(yin_frames, np.float64), sess.input_raw(parabolic_shifts, np.float64), clips, n_lags, n_frames, lp_ptr, vp_ptr, sr=sr, fmin=fmin,
                      min_period=min_period, n_thresholds=n_thresholds, beta_parameters=beta_parameters, boltzmann_parameter=boltzmann_parameter, n_pitch_bins=n_pitch_bins,
                      n_bins_per_semitone=n_bins_per_semitone, no_trough_prob=no_trough_prob)
        log_prob, voiced_prob = sess.result(lp_h), sess.result(vp_h)
    finally:
        sess.close()
    return _arrays.swap_last_two(log_prob.reshape(lead + (n_frames, 2 * n_pitch_bins))), voiced_prob.reshape(lead + (n_frames,))


def _pyin_decoder(n_pitch_bins, n_bins_per_semitone, max_transition_rate, hop, sr, switch_prob, transition_min_prob):
    """The decoder of the reference's transition and ``p_init`` (``core/pitch.py:827-842``); its host tables are kept for the next call."""
    from .. import sequence as _sequence

    key = (n_pitch_bins, n_bins_per_semitone, max_transition_rate, hop, sr, switch_prob, transition_min_prob)
    if key not in _PYIN_DECODERS:
        max_semitones_per_frame = round(max_transition_rate * 12 * hop / sr)
        transition_width = max_semitones_per_frame * n_bins_per_semitone + 1
        transition = _sequence.transition_local(n_pitch_bins, transition_width, window="triangle", wrap=False)
        transition = np.kron(_sequence.transition_loop(2, 1 - switch_prob), transition)
        p_init = np.ones(2 * n_pitch_bins) / (2 * n_pitch_bins)
        decoder = _sequence._ResidentDecoder(transition, p_init, transition_min_prob)
        if len(_PYIN_DECODERS) >= 4:
            _PYIN_DECODERS.clear()
        _PYIN_DECODERS[key] = decoder
    return _PYIN_DECODERS[key]


def _pyin_run(y, fmin, fmax, sr, frame_length, hop_length, n_thresholds, beta_parameters, boltzmann_parameter, resolution, max_transition_rate, switch_prob, no_trough_prob, fill_na, center,
              pad_mode, transition_min_prob):
    from .. import sequence as _sequence

    y, real, hop, center, pad_mode, min_period, max_period = _yin_prepare(y, fmin, fmax, sr, frame_length, hop_length, center, pad_mode)
    n_bins_per_semitone, n_pitch_bins = _pyin_bins(fmin, fmax, resolution, n_thresholds, boltzmann_parameter)
    n_states = 2 * n_pitch_bins
    decoder = _pyin_decoder(n_pitch_bins, n_bins_per_semitone, max_transition_rate, hop, sr, switch_prob, transition_min_prob)
    freqs = fmin * 2 ** (np.arange(n_pitch_bins) / (12 * n_bins_per_semitone))
    lead = tuple(int(s) for s in y.shape[:-1])
    n = int(y.shape[-1])
    batch = int(np.prod(lead, dtype=np.int64)) if lead else 1
    n_frames = 1 + (n + (2 * (frame_length // 2) if center else 0) - frame_length) // hop
    n_lags = max_period - min_period + 1
    f64 = np.dtype(np.float64)
    y = _arrays.cast(y, f64).reshape((batch, n))   # float32 samples are widened exactly: the front half computes in float64 after the load anyway
    # whole clips per chunk: the front half (16 bytes per lag and frame), log_prob (8 per state and step) and the pointer scratch (2)
    per_clip = (16 * n_lags + 10 * n_states) * n_frames
    chunk = int(max(1, min(batch, _sequence.SCRATCH_BUDGET // per_clip)))
    parts = []
    for c0 in range(0, max(batch, 1), chunk):   # (an empty batch takes the same path: every native call answers an empty one)
        c1 = min(batch, c0 + chunk)
        clips = c1 - c0
        cm, sh, _ = _yin_launch(y[c0:c1], f64, _YIN_FRAMES, sr, frame_length, hop, 0.0, center, pad_mode, min_period, max_period)
        sess = _arrays.Session(cm)
        try:
            lp_ptr = sess.scratch(8 * clips * n_states * n_frames)
            ptr_ptr = sess.scratch(2 * clips * n_states * n_frames)
            vp_ptr, vp_h = sess.output((clips, n_frames), np.float64)
            f0_ptr, f0_h = sess.output((clips, n_frames), np.float64)
            flag_ptr, flag_h = sess.output((clips, n_frames), np.uint8)
            _pyin_obs(sess, sess.input_raw(cm, f64), sess.input_raw(sh, f64), clips, n_lags, n_frames, lp_ptr, vp_ptr, sr=sr, fmin=fmin, min_period=min_period, n_thresholds=n_thresholds,
                      beta_parameters=beta_parameters, boltzmann_parameter=boltzmann_parameter, n_pitch_bins=n_pitch_bins, n_bins_per_semitone=n_bins_per_semitone,
                      no_trough_prob=no_trough_prob)
            del cm, sh
            states_ptr, _ = decoder.run(sess, lp_ptr, ptr_ptr, clips, n_frames)
            sess.ctx.pyin_finish_exec(states_ptr, clips * n_frames, n_pitch_bins, sess.input_raw(_spectrum._as_like(sess, freqs), f64), fill_na, f0_ptr, flag_ptr)
            parts.append((sess.result(f0_h), sess.result(flag_h), sess.result(vp_h)))
        finally:
            sess.close()
    if len(parts) > 1:
        if is_torch_tensor(parts[0][0]):
            import torch

            parts = [tuple(torch.cat([p[i] for p in parts]) for i in range(3))]
        else:
            parts = [tuple(np.concatenate([p[i] for p in parts]) for i in range(3))]
    f0, flag, voiced_prob = parts[0]
    if is_torch_tensor(flag):
        import torch

        flag = flag.view(torch.bool)
    else:
        flag = flag.view(np.bool_)
    return f0.reshape(lead + (n_frames,)), flag.reshape(lead + (n_frames,)), voiced_prob.reshape(lead + (n_frames,))


def pyin(y, *, fmin, fmax, sr=22050, frame_length=2048, hop_length=None, n_thresholds=100, beta_parameters=(2, 18), boltzmann_parameter=2, resolution=0.1, max_transition_rate=35.92,
         switch_prob=0.01, no_trough_prob=0.01, fill_na=np.nan, center=True, pad_mode="constant", transition_min_prob=1e-4):
    """Fundamental frequency estimation with probabilistic YIN; drop-in for ``librosa.pyin`` (``core/pitch.py:631-852``).

    ``y``: (..., n) NumPy array or device tensor, float32 or float64.  Returns ``(f0, voiced_flag, voiced_prob)`` of shape (..., n_frames): float64,
    bool and float64, NumPy arrays for NumPy input and device tensors for a device tensor.  ``y`` is never written.  See the module docstring
    for the pipeline and the documented differences."""
    return _pyin_run(y, fmin, fmax, sr, frame_length, hop_length, n_thresholds, beta_parameters, boltzmann_parameter, resolution, max_transition_rate, switch_prob, no_trough_prob, fill_na,
                     center, pad_mode, transition_min_prob)
