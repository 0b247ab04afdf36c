"""``chroma_stft`` and ``chroma_cqt`` with librosa's signatures (``librosa/feature/spectral.py:1137-1293, 1296-1423``).

Both end in the same device launch (``csrc/lra_chroma.h``, ``lra_chroma_exec``): the dense projection ``raw[c, t] = sum_f W[c, f] X[f, t]``,
``chroma_cqt``'s threshold and ``util.normalize(raw, norm=norm, axis=-2)``, reading the spectrogram once and writing only the ``n_chroma``
rows.  With ``y`` given the front end -- the power STFT, or ``cqt`` and its magnitude -- runs on the device first and nothing but the chroma
comes back.  The filter banks are host tables (``filters.chroma`` / ``filters.cq_to_chroma``, bit-identical to the reference's).

Norms ``inf``, ``1``, ``2`` and ``None`` are normalised by the kernel; any other norm (``-inf``, ``0``, a general ``p``) takes the kernel's
unnormalised result through the host ``util.normalize``.  A non-finite value raises ``ParameterError("Input must be finite")`` for every norm,
``None`` included, as the reference's ``normalize`` does.

Not provided: ``tuning=None`` (the reference's default: it estimates the tuning with its pitch tracker, ``estimate_tuning`` / ``piptrack``,
which these functions do not call) -- pass a number: ``tuning=librosa_amd.estimate_tuning(y=y, sr=sr)`` supplies the number on the device; ``chroma_cqt(cqt_mode="hybrid")``; complex ``S`` / ``C``.
"""
from __future__ import annotations

import hashlib

import numpy as np

from .. import _arrays
from .. import filters
from ..core import constantq as _constantq
from ..core import spectrum as _spectrum
from ..util import utils as util
from ..util.exceptions import ParameterError
from ..util.utils import is_torch_tensor

__all__ = ["chroma_stft", "chroma_cqt"]

# the converter chroma_cqt(y=...) hands to cqt between octaves: the reference's default (see core/constantq.py for what it runs as here)
CQT_RES_TYPE = "soxr_hq"

_NO_TUNING = "tuning=None (automatic tuning estimation) is not provided by librosa_amd; pass a number"


def _norm_code(norm):
    """The kernel's code for ``norm``, or None when the host ``util.normalize`` has to do it; a norm that ``normalize`` refuses
    (``util/utils.py:1000-1001``) is refused here, before any device work."""
    if norm is None:
        return 0
    number = isinstance(norm, (int, float, np.number)) and not isinstance(norm, (bool, np.bool_))
    if not (number and (norm > 0 or norm == 0 or np.isneginf(norm))):
        raise ParameterError(f"Unsupported norm: {norm!r}")
    if norm == 1:
        return 1
    if norm == 2:
        return 2
    if np.isposinf(norm):
        return 3
    return None


def _host_normalize(res, norm):
    host = res.detach().cpu().numpy() if is_torch_tensor(res) else res
    normed = util.normalize(host, norm=norm, axis=-2)
    return _arrays._torch().from_numpy(np.ascontiguousarray(normed)).to(res.device) if is_torch_tensor(res) else normed


def _bank_ptr(sess, bank, real):
    """Device pointer of the bank in the compute dtype: kept in the context under the table's digest, or uploaded for this call."""
    ctx = sess.ctx
    table = np.ascontiguousarray(bank, dtype=real)
    if ctx.table_cacheable(table.nbytes):
        return ctx.device_table(("chroma_bank", real.str, table.shape, hashlib.sha1(table.tobytes()).hexdigest()), lambda: table)
    return sess.input_raw(_spectrum._as_like(sess, table), real)


def _project(sess, x_ptr, batch, n_bins, n_frames, strides, real, bank, code, threshold):
    """One launch on a resident spectrogram; returns (result handle, non-finite flag).  ``strides``: (batch, bin, frame) in elements."""
    n_chroma = int(bank.shape[0])
    out_ptr, handle = sess.output((batch, n_chroma, n_frames), real)
    if batch * n_chroma * n_frames == 0:
        return handle, False
    w_ptr = _bank_ptr(sess, bank, real) if n_bins else 0
    flagged = sess.ctx.chroma_exec(x_ptr, batch, n_bins, n_frames, strides[0], strides[1], strides[2], real, w_ptr, n_chroma, code, threshold, out_ptr, sess.scratch(256))
    return handle, flagged


def _apply_bank(X, bank, norm, threshold, what):
    """``normalize(threshold(einsum("cf,...ft->...ct", bank, X)))`` of a given (..., n_bins, n_frames) array or device tensor."""
    x_dtype = _arrays.numpy_dtype_of(X)
    if x_dtype.kind == "c":
        raise ParameterError(f"{what} must be real-valued")
    if X.ndim < 2:
        raise ParameterError(f"{what} must have at least 2 dimensions, given shape={tuple(X.shape)}")
    real = np.dtype(np.float64) if (x_dtype == np.float64 or bank.dtype == np.float64) else np.dtype(np.float32)
    lead = tuple(int(s) for s in X.shape[:-2])
    n_bins, n_frames = int(X.shape[-2]), int(X.shape[-1])
    if n_bins != bank.shape[1]:
        raise ParameterError(f"{what} has {n_bins} bins but the filter bank expects {bank.shape[1]}")
    batch = int(np.prod(lead, dtype=np.int64)) if lead else 1
    code = _norm_code(norm)
    sess = _arrays.Session(X)
    try:
        Xt = _arrays.swap_last_two(X)  # (..., t, f)
        rows = None
        if batch * n_frames * n_bins == 0:
            x_ptr, strides = 0, (0, 0, 0)
        elif is_torch_tensor(X):
            rows = _spectrum._frame_major_strides(Xt, n_bins) if Xt.dtype == _arrays.torch_dtype(real) else None
            if rows is not None:
                # the device layout [b][t][f], rows possibly padded to whole cache lines (what _spectrogram / stft(...).abs() ** 2 return): in place
                sess._keep.append(Xt)
                x_ptr, strides = Xt.data_ptr(), (rows[0], 1, rows[1])
            elif Xt.is_contiguous():
                x_ptr, strides = sess.input_raw(Xt, real), (n_frames * n_bins, 1, n_bins)
            else:
                x_ptr, strides = sess.input_raw(X, real), (n_bins * n_frames, n_frames, 1)
        elif Xt.flags["C_CONTIGUOUS"] and n_frames > 1:
            x_ptr, strides = sess.input_raw(Xt, real), (n_frames * n_bins, 1, n_bins)   # a view of the device layout (what our own _spectrogram returns)
        else:
            x_ptr, strides = sess.input_raw(X, real), (n_bins * n_frames, n_frames, 1)  # the reference's layout: bins major, frames contiguous
        handle, flagged = _project(sess, x_ptr, batch, n_bins, n_frames, strides, real, bank, 0 if code is None else code, threshold)
        if flagged:
            raise ParameterError("Input must be finite")
        res = sess.result(handle)
    finally:
        sess.close()
    res = res.reshape(lead + (int(bank.shape[0]), n_frames))
    return _host_normalize(res, norm) if code is None else res


def chroma_stft(*, y=None, sr=22050, S=None, norm=np.inf, n_fft=2048, hop_length=512, win_length=None, window="hann", center=True, pad_mode="constant", tuning=None,
                n_chroma=12, check_finite=True, **kwargs):
    """Chromagram of a waveform or a power spectrogram; drop-in for ``librosa.feature.chroma_stft`` (``feature/spectral.py:1137-1293``).

    ``kwargs`` go to ``filters.chroma`` (``ctroct, octwidth, norm, base_c, dtype``).  With ``y`` the power STFT (fused, mixed-radix or rocFFT,
    whichever serves ``n_fft``) and the chroma kernel run back to back on the device; the ``(..., 1 + n_fft // 2, n_frames)`` spectrogram is
    never downloaded.  With ``S`` (a power spectrogram, NumPy array or device tensor) only the chroma kernel runs; the view ``_spectrogram``
    returns for device tensors is read in place.  The result has the dtype of ``S`` / ``y`` (float64 when the bank is: ``dtype=np.float64``).

    Not provided: ``tuning=None`` -- the reference's default, which estimates the tuning from the spectrogram with its pitch tracker
    (``estimate_tuning``).  Pass a number (``0.0``: A440); ``tuning=librosa_amd.estimate_tuning(y=y, sr=sr)`` supplies the number on the device.  ``check_finite`` (an extension, as for ``stft``) controls the scan of a device ``y``.
    """
    if tuning is None:
        raise ParameterError(_NO_TUNING)
    if S is not None:
        if n_fft is None or n_fft // 2 + 1 != S.shape[-2]:
            n_fft = 2 * (S.shape[-2] - 1)
        _norm_code(norm)
        bank = filters.chroma_cached(sr=sr, n_fft=n_fft, tuning=tuning, n_chroma=n_chroma, **kwargs)
        return _apply_bank(S, bank, norm, None, "S")
    if n_fft is None:
        raise ParameterError(f"Unable to compute spectrogram with n_fft={n_fft}")
    if y is None:
        raise ParameterError("Input signal must be provided to compute a spectrogram")
    code = _norm_code(norm)
    bank = filters.chroma_cached(sr=sr, n_fft=n_fft, tuning=tuning, n_chroma=n_chroma, **kwargs)
    if bank.dtype == np.float64 and _arrays.numpy_dtype_of(y) != np.float64:
        # a float64 bank over float32 audio: the float32 spectrogram is widened on its way into the kernel, which the chained form does not do
        S, _ = _spectrum._spectrogram(y=y, n_fft=n_fft, hop_length=hop_length, power=2, win_length=win_length, window=window, center=center, pad_mode=pad_mode)
        return _apply_bank(S, bank, norm, None, "S")

    def post(sess, s_ptr, batch, n_bins, n_frames, pitch, real):
        handle, flagged = _project(sess, s_ptr, batch, n_bins, n_frames, (n_frames * pitch, 1, pitch), real, bank, 0 if code is None else code, None)
        if flagged:
            if (check_finite or not is_torch_tensor(y)) and not _spectrum._all_finite(y):
                raise ParameterError("Audio buffer is not finite everywhere")
            raise ParameterError("Input must be finite")
        return handle, int(bank.shape[0])

    res = _spectrum._run_stft_family("power", y, n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window, center=center, pad_mode=pad_mode, power=2.0,
                                     check_finite=check_finite, post=post)
    return _host_normalize(res, norm) if code is None else res


def chroma_cqt(*, y=None, sr=22050, C=None, hop_length=512, fmin=None, norm=np.inf, threshold=0.0, tuning=None, n_chroma=12, n_octaves=7, window=None, bins_per_octave=36,
               cqt_mode="full"):
    """Constant-Q chromagram; drop-in for ``librosa.feature.chroma_cqt`` (``feature/spectral.py:1296-1423``).

    With ``y``: ``cqt`` (``n_octaves * bins_per_octave`` bins), its magnitude and the chroma kernel run on the device, nothing in between is
    downloaded.  With ``C`` (constant-Q magnitudes, NumPy array or device tensor) only the chroma kernel runs.  ``threshold``: raw chroma
    values below it are set to zero before the normalisation (``None``: no threshold).  ``window`` goes to ``filters.cq_to_chroma``.

    Not provided: ``tuning=None`` with ``y`` -- the reference's default, which estimates the tuning with its pitch tracker; pass a number --
    ``tuning=librosa_amd.estimate_tuning(y=y, sr=sr)`` supplies the number on the device --
    (``C`` given, ``tuning`` is not used, as in the reference) -- and ``cqt_mode="hybrid"``.
    """
    if bins_per_octave is None:
        bins_per_octave = n_chroma
    elif np.remainder(bins_per_octave, n_chroma) != 0:
        raise ParameterError(f"bins_per_octave={bins_per_octave} must be an integer multiple of n_chroma={n_chroma}")
    _norm_code(norm)
    if C is not None:
        if C.ndim < 2:
            raise ParameterError(f"C must have at least 2 dimensions, given shape={tuple(C.shape)}")
        bank = filters.cq_to_chroma_cached(int(C.shape[-2]), bins_per_octave=bins_per_octave, n_chroma=n_chroma, fmin=fmin, window=window)
        return _apply_bank(C, bank, norm, threshold, "C")
    if cqt_mode != "full":
        raise ParameterError(f"cqt_mode={cqt_mode!r} is not provided by librosa_amd.feature.chroma_cqt; only 'full'")
    if y is None:
        raise ParameterError("At least one of C or y must be provided to compute chroma")
    if tuning is None:
        raise ParameterError(_NO_TUNING)
    n_bins = int(n_octaves * bins_per_octave)
    bank = filters.cq_to_chroma_cached(n_bins, bins_per_octave=bins_per_octave, n_chroma=n_chroma, fmin=fmin, window=window)
    code = _norm_code(norm)

    def post(sess, c_ptr, batch, n_frames, n_cq, real):
        mag_ptr = sess.scratch(batch * n_frames * n_cq * real.itemsize)
        sess.ctx.magnitude_exec(c_ptr, mag_ptr, batch * n_frames * n_cq, real)
        handle, flagged = _project(sess, mag_ptr, batch, n_cq, n_frames, (n_frames * n_cq, 1, n_cq), real, bank, 0 if code is None else code, threshold)
        if flagged:
            raise ParameterError("Audio buffer is not finite everywhere" if not _spectrum._all_finite(y) else "Input must be finite")
        return handle, int(bank.shape[0])

    # (a float64 bank -- a float64 ``window`` -- gives a float64 result in the reference: the transform then runs in double precision as a whole)
    res = _constantq.cqt(y, sr=sr, hop_length=hop_length, fmin=fmin, n_bins=n_bins, bins_per_octave=bins_per_octave, tuning=tuning, res_type=CQT_RES_TYPE,
                         dtype=np.complex128 if bank.dtype == np.float64 else None, _post=post)
    return _host_normalize(res, norm) if code is None else res
