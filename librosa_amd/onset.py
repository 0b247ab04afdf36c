"""Spectral-flux onset strength: ``onset_strength`` / ``onset_strength_multi`` with librosa's signatures
(``librosa/onset.py:217-367, 445-645``).

With the default feature (the mel spectrogram) the whole chain runs on the device in three launches: the fused mel kernel, the per-clip
maximum behind ``power_to_db``'s ``top_db`` floor, and the flux kernel (``csrc/lra_onset.h``), which applies the decibel scaling, the band
max filter (``max_size``), the lag difference, the rectification, the channel aggregation, the left padding and the trim while it reads
the mel power spectrogram.  Only the ``(..., n_channels, n_frames)`` envelope comes back.  ``detrend=True`` adds one row-recurrence launch
and returns float64, as the reference does.  With ``S`` given (or another ``feature`` callable) the same flux kernel runs on that
spectrogram.  ``np.mean`` / ``np.sum`` / ``np.max`` / ``np.min`` / ``np.median`` and ``aggregate=False`` run on the device; any other
aggregate callable is a slow path: the device computes the rectified per-band flux, the callable is applied on the host exactly as
``util.sync`` applies it, and the padding / trim / detrend run on the device again.  Device tensors in give device tensors out.
"""
from __future__ import annotations

import numpy as np

from . import _arrays, filters
from .core import spectrum as _spectrum
from .feature import spectral as _spectral
from .util import utils as util
from .util.exceptions import ParameterError
from .util.utils import is_torch_tensor

__all__ = ["onset_strength", "onset_strength_multi"]

# aggregation codes of lra_onset_exec (include/librosa_amd.h)
_NONE, _MEAN, _SUM, _MAX, _MIN, _MEDIAN, _ROWS = range(7)
_DEVICE_AGGREGATES = ((np.mean, _MEAN), (np.sum, _SUM), (np.max, _MAX), (np.amax, _MAX), (np.min, _MIN), (np.amin, _MIN), (np.median, _MEDIAN))

# power_to_db's defaults, the scaling the reference applies to the feature (onset.py:579-583)
_AMIN, _TOP_DB = 1e-10, 80.0


def onset_strength(*, y=None, sr=22050, S=None, lag=1, max_size=1, ref=None, detrend=False, center=True, feature=None, aggregate=None, **kwargs):
    """Spectral flux onset strength envelope; drop-in for ``librosa.onset.onset_strength`` (``librosa/onset.py:217-367``).

    ``mean_f max(0, S[f, t] - ref[f, t - lag])`` with ``S = power_to_db(melspectrogram(y))`` by default; see the module docstring for
    what runs where.  Returns ``(..., n_frames)``."""
    if aggregate is False:
        raise ParameterError("aggregate parameter cannot be False when computing full-spectrum onset strength.")
    odf_all = onset_strength_multi(y=y, sr=sr, S=S, lag=lag, max_size=max_size, ref=ref, detrend=detrend, center=center, feature=feature, aggregate=aggregate, channels=None,
                                   **kwargs)
    return odf_all[..., 0, :]


def onset_strength_multi(*, y=None, sr=22050, S=None, n_fft=2048, hop_length=512, lag=1, max_size=1, ref=None, detrend=False, center=True, feature=None, aggregate=None,
                         channels=None, **kwargs):
    """Spectral flux onset strength per channel; drop-in for ``librosa.onset.onset_strength_multi`` (``librosa/onset.py:445-645``).

    Returns ``(..., n_channels, n_frames)`` (``(..., n_bands, n_frames)`` for ``aggregate=False``), in ``S``'s precision, or float64 with
    ``detrend=True``.  A caller's ``ref`` is read in ``S``'s precision."""
    fused = S is None and (feature is None or feature is _spectral.melspectrogram)
    if feature is None:
        feature = _spectral.melspectrogram
        kwargs.setdefault("fmax", 0.5 * sr)
    if aggregate is None:
        aggregate = np.mean
    if not util.is_positive_int(lag):
        raise ParameterError(f"lag={lag} must be a positive integer")
    if not util.is_positive_int(max_size):
        raise ParameterError(f"max_size={max_size} must be a positive integer")
    # onset.py:612-622: aggregation only for a callable; channels=None is one channel over every band (padded boundaries)
    code = _NONE
    if callable(aggregate):
        code = next((c for f, c in _DEVICE_AGGREGATES if aggregate is f), None)  # None: a host callable (the slow path)
    pad_width = lag + (n_fft // (2 * hop_length) if center else 0)  # onset.py:624-628
    job = dict(lag=lag, max_size=max_size, code=code, aggregate=aggregate, channels=channels, pad_width=pad_width, center=center, detrend=bool(detrend))
    if fused:
        return _fused(y, sr, n_fft, hop_length, ref, job, kwargs)
    if S is None:
        S = feature(y=y, sr=sr, n_fft=n_fft, hop_length=hop_length, **kwargs)
        return _given(S, ref, job, db=True)
    return _given(S, ref, job, db=False)


# ---- channels: util.sync's boundaries (util/utils.py:1785-1814, index_to_slice :1646-1687, fix_frames :613-677) ----------------------
def _fix_frames(frames, x_min, x_max, pad):
    frames = np.asarray(frames)
    if np.any(frames < 0):
        raise ParameterError("Negative frame index detected")
    if pad:
        frames = np.clip(frames, x_min, x_max)
        frames = np.concatenate((np.asarray([x_min, x_max]), frames))
    frames = frames[frames >= x_min]
    frames = frames[frames <= x_max]
    return np.unique(frames).astype(int)


def _channel_slices(channels, n_bands):
    pad = channels is None
    idx = [slice(None)] if channels is None else channels
    if np.all([isinstance(c, slice) for c in idx]):
        return list(idx)
    if np.all([np.issubdtype(type(c), np.integer) for c in idx]):
        bounds = _fix_frames(np.asarray(idx), 0, n_bands, pad)
        return [slice(int(a), int(b)) for a, b in zip(bounds[:-1], bounds[1:])]
    raise ParameterError(f"Invalid index set: {idx}")


def _channel_tables(slices, n_bands, code):
    """Channels -> (offsets, band indices, largest channel) int32 tables: each channel's bands in the order its slice visits them."""
    bands = [np.arange(n_bands)[s] for s in slices]
    if code in (_MAX, _MIN) and any(len(b) == 0 for b in bands):
        name = "maximum" if code == _MAX else "minimum"
        raise ValueError(f"zero-size array to reduction operation {name} which has no identity")  # what np.max / np.min raise on an empty channel
    off = np.zeros(len(bands) + 1, np.int32)
    off[1:] = np.cumsum([len(b) for b in bands])
    idx = np.concatenate(bands).astype(np.int32) if bands and off[-1] else np.zeros(1, np.int32)
    return off, idx, max((len(b) for b in bands), default=0)


def _prepare_channels(job, n_bands):
    """The channel tables of a device aggregate, checked before any device work."""
    if job["code"] not in (None, _NONE):
        tables = _channel_tables(_channel_slices(job["channels"], n_bands), n_bands, job["code"])
        job["tables"] = None if job["channels"] is None else tables  # channels=None: every band in order, no tables to upload
    elif job["code"] is None:
        _channel_slices(job["channels"], n_bands)


def _out_frames(n_env, job, n_frames):
    """onset.py:624-642: ``pad_width`` zeros on the left, then (center) trimmed to the spectrogram's frame count."""
    total = n_env + job["pad_width"]
    return min(total, n_frames) if job["center"] else total


# ---- device work ----------------------------------------------------------------------------------------------------------------------
def _envelope(sess, s_ptr, ref_ptr, batch, n_bands, n_frames, real, job, item_max_ptr):
    """The flux kernel on a [batch][n_bands][n_frames] spectrogram -> (handle, rows, cols).  For a host aggregate callable: the rectified
    per-band flux, unpadded (the caller aggregates it and comes back through ``_finish_rows``)."""
    ctx = sess.ctx
    lag = job["lag"]
    n_env = max(n_frames - lag, 0)
    code = job["code"]
    if code is None:
        out_ptr, handle = sess.output((batch, n_bands, n_env), real)
        ctx.onset_exec(s_ptr, ref_ptr, out_ptr, batch, n_bands, n_frames, real, lag, job["max_size"], _NONE, None, None, 0, 0, 0, n_env, item_max_ptr=item_max_ptr,
                       amin=_AMIN, top_db=_TOP_DB)
        return handle, n_bands, n_env
    n_out = _out_frames(n_env, job, n_frames)
    off_ptr = band_ptr = None
    n_ch = max_ch = 0
    rows = n_bands
    if code != _NONE and job["tables"] is None:
        n_ch, max_ch, rows = 1, n_bands, 1
    elif code != _NONE:
        off, idx, max_ch = job["tables"]
        n_ch = rows = len(off) - 1
        off_ptr = sess.input_raw(_spectrum._as_like(sess, off), np.int32)
        band_ptr = sess.input_raw(_spectrum._as_like(sess, idx), np.int32)
    out_dtype = np.dtype(np.float64) if job["detrend"] else real
    stage = job.get("stage")
    if stage is None:
        out_ptr, handle = sess.output((batch, rows, n_out), out_dtype)
    else:
        out_ptr = sess.scratch(max(batch * rows * n_out, 1) * out_dtype.itemsize)  # the envelope stays on the device for the caller's stage
    env_ptr = sess.scratch(max(batch * rows * n_out, 1) * real.itemsize) if job["detrend"] else None
    ctx.onset_exec(s_ptr, ref_ptr, out_ptr, batch, n_bands, n_frames, real, lag, job["max_size"], code, off_ptr, band_ptr, n_ch, max_ch, job["pad_width"], n_out,
                   item_max_ptr=item_max_ptr, amin=_AMIN, top_db=_TOP_DB, detrend_env_ptr=env_ptr)
    if stage is not None:
        return stage(sess, out_ptr, batch * rows, n_out, out_dtype)
    return handle, rows, n_out


def _sync_host(flux, job):
    """util.sync(flux, channels, aggregate=callable, pad=channels is None, axis=-2) on the host (util/utils.py:1785-1814)."""
    slices = _channel_slices(job["channels"], flux.shape[-2])
    agg = np.empty(flux.shape[:-2] + (len(slices), flux.shape[-1]), dtype=flux.dtype)
    for i, s in enumerate(slices):
        agg[..., i, :] = job["aggregate"](flux[..., s, :], axis=-2)
    return agg


def _finish_rows(agg, n_frames, job, like):
    """The host-aggregated rows back through the kernel's padding / trim / detrend (aggregate code ROWS)."""
    real = np.dtype(np.float32) if agg.dtype == np.float32 else np.dtype(np.float64)
    lead, n_ch, n_env = agg.shape[:-2], int(agg.shape[-2]), int(agg.shape[-1])
    batch = int(np.prod(lead, dtype=np.int64)) if lead else 1
    n_out = _out_frames(n_env, job, n_frames)
    sess = _arrays.Session(like if is_torch_tensor(like) else np.empty(0))
    try:
        a_ptr = sess.input_raw(_spectrum._as_like(sess, np.ascontiguousarray(agg, dtype=real).reshape(batch, n_ch, n_env)), real)
        out_ptr, handle = sess.output((batch, n_ch, n_out), np.float64 if job["detrend"] else real)
        env_ptr = sess.scratch(max(batch * n_ch * n_out, 1) * real.itemsize) if job["detrend"] else None
        sess.ctx.onset_exec(a_ptr, None, out_ptr, batch, n_ch, n_env, real, 1, 1, _ROWS, None, None, 0, 0, job["pad_width"], n_out, detrend_env_ptr=env_ptr)
        res = sess.result(handle)
    finally:
        sess.close()
    return res.reshape(lead + (n_ch, n_out))


def _slow_path(flux, n_frames, job):
    host = flux.detach().cpu().numpy() if is_torch_tensor(flux) else flux
    return _finish_rows(_sync_host(host, job), n_frames, job, flux)


def _check_ref_shape(ref, shape):
    if tuple(ref.shape) != tuple(shape):
        raise ParameterError(f"Reference spectrum shape {tuple(ref.shape)} must match input spectrum {tuple(shape)}")


def _fused(y, sr, n_fft, hop_length, ref, job, kwargs):
    """melspectrogram(y) -> power_to_db -> flux, without the mel leaving the device (``_run_stft_family``'s ``post`` hook, as feature.mfcc)."""
    if y is None:
        raise ParameterError("Input signal must be provided to compute a spectrogram")
    if n_fft is None:
        raise ParameterError(f"Unable to compute spectrogram with n_fft={n_fft}")
    kw = dict(kwargs)
    win_length = kw.pop("win_length", None)
    window = kw.pop("window", "hann")
    pad_mode = kw.pop("pad_mode", "constant")
    power = kw.pop("power", 2.0)
    check_finite = kw.pop("check_finite", True)
    mel_basis = filters.mel_cached(sr=sr, n_fft=n_fft, **kw)
    _prepare_channels(job, int(mel_basis.shape[0]))
    if ref is not None:
        # the mel is always centred (onset.py:580 does not forward `center`): its shape is known before any device work
        n = int(y.shape[-1])
        _check_ref_shape(ref, tuple(y.shape[:-1]) + (int(mel_basis.shape[0]), 1 + (n + 2 * (n_fft // 2) - n_fft) // int(hop_length)))

    def post(sess, mel_ptr, batch, n_mels, n_frames, real):
        ctx = sess.ctx
        max_ptr = sess.scratch(batch * real.itemsize)
        ctx.item_max_exec(mel_ptr, batch, n_mels * n_frames, real, max_ptr, absolute=True)  # power_to_db(np.abs(S)): top_db's per-clip maximum
        ref_ptr = None
        if ref is not None:
            r = ref if is_torch_tensor(ref) else _spectrum._as_like(sess, np.asarray(ref))
            ref_ptr = sess.input_raw(r, real)
        return _envelope(sess, mel_ptr, ref_ptr, batch, n_mels, n_frames, real, job, max_ptr)

    res = _spectrum._run_stft_family("mel", y, n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window, center=True, pad_mode=pad_mode, power=float(power),
                                     mel_basis=mel_basis, check_finite=check_finite, post=post)
    if job["code"] is None:
        n = int(y.shape[-1])
        return _slow_path(res, 1 + (n + 2 * (n_fft // 2) - n_fft) // int(hop_length), job)
    return res


def _strength_then(y, *, sr, hop_length, stage, aggregate=np.mean):
    """``onset_strength(y=y, sr=sr, hop_length=hop_length, aggregate=aggregate)`` (every other argument at its default; ``aggregate`` one of
    the device aggregates) without downloading the envelope: ``stage(sess, env_ptr, rows, n, dtype) -> (handle, rows, cols)`` runs further
    device work on the ``[rows][n]`` envelope (one row per clip) and its result comes back as ``(..., rows, cols)`` (``feature.tempogram`` /
    ``tempo``; ``beat.beat_track`` with ``np.median``)."""
    n_fft = 2048
    code = next(c for f, c in _DEVICE_AGGREGATES if aggregate is f)
    job = dict(lag=1, max_size=1, code=code, aggregate=aggregate, channels=None, pad_width=1 + n_fft // (2 * hop_length), center=True, detrend=False, stage=stage)
    return _fused(y, sr, n_fft, hop_length, None, job, {"fmax": 0.5 * sr})


def _given(S, ref, job, db):
    """A spectrogram from the caller (``db=False``: used as given) or from another feature callable (``db=True``: ``power_to_db(|S|)``
    is applied by the flux kernel as it reads S)."""
    on_device = is_torch_tensor(S)
    if not on_device:
        S = np.asarray(S)
    dt = _arrays.numpy_dtype_of(S)
    if dt.kind == "c":
        if not db:
            raise ParameterError("S must be a real-valued spectrogram")
        S = S.abs() if on_device else np.abs(S)  # np.abs(feature(...)) (onset.py:580)
        dt = _arrays.numpy_dtype_of(S)
    if S.ndim < 2:  # np.atleast_2d (onset.py:589)
        S = S.reshape((1,) * (2 - S.ndim) + tuple(S.shape))
    if ref is not None:
        if not is_torch_tensor(ref):
            ref = np.asarray(ref)
        _check_ref_shape(ref, S.shape)
    real = np.dtype(np.float32) if dt == np.float32 else np.dtype(np.float64)
    lead = tuple(S.shape[:-2])
    n_bands, n_frames = int(S.shape[-2]), int(S.shape[-1])
    batch = int(np.prod(lead, dtype=np.int64)) if lead else 1
    _prepare_channels(job, n_bands)
    sess = _arrays.Session(S if on_device else np.empty(0))
    try:
        ctx = sess.ctx
        s_ptr = sess.input_raw(S.reshape(batch, n_bands, n_frames), real)
        ref_ptr = None
        if ref is not None:
            r = ref if is_torch_tensor(ref) else _spectrum._as_like(sess, ref)
            ref_ptr = sess.input_raw(r.reshape(batch, n_bands, n_frames), real)
        max_ptr = None
        if db:
            max_ptr = sess.scratch(max(batch, 1) * real.itemsize)
            if batch * n_bands * n_frames:
                ctx.item_max_exec(s_ptr, batch, n_bands * n_frames, real, max_ptr, absolute=True)
        handle, rows, cols = _envelope(sess, s_ptr, ref_ptr, batch, n_bands, n_frames, real, job, max_ptr)
        res = sess.result(handle).reshape(lead + (rows, cols))
    finally:
        sess.close()
    if job["code"] is None:
        return _slow_path(res, n_frames, job)
    return res
