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

``onset_detect`` (``librosa/onset.py:31-214``) picks peaks of that envelope with ``csrc/lra_peaks.h``.  From ``y`` the envelope never leaves
the device: the normalisation, the candidate flags and the selection run as a stage behind the flux kernel, and only the ``uint8`` onset row
comes back (with ``backtrack=True`` also the ``int32`` row of preceding minima, ``onset_backtrack``'s table, ``:370-441``).
"""
from __future__ import annotations

import numpy as np

from . import _arrays, filters
from .core import convert as _convert
from .core import spectrum as _spectrum
from .feature import spectral as _spectral
from .util import peaks as _peaks
from .util import utils as util
from .util.exceptions import ParameterError
from .util.utils import is_torch_tensor

__all__ = ["onset_detect", "onset_strength", "onset_strength_multi", "onset_backtrack"]

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


# ---- onset_detect / onset_backtrack ---------------------------------------------------------------------------------------------------
_PICK_KEYS = ("pre_max", "post_max", "pre_avg", "post_avg", "wait", "delta", "method")


def onset_detect(*, y=None, sr=22050, onset_envelope=None, hop_length=512, backtrack=False, energy=None, units="frames", normalize=True, sparse=True, **kwargs):
    """Onset events by peak picking on the onset strength envelope; drop-in for ``librosa.onset.onset_detect`` (``librosa/onset.py:31-214``).

    ``sparse=True`` (one-dimensional input only): ``int64`` frame indices, or samples / seconds with ``units``; ``sparse=False``: a bool array
    of the envelope's shape.  ``kwargs`` go to ``util.peak_pick``; the defaults are the reference's (30 ms / 0 ms maximum windows, 100 ms /
    100 ms mean windows, 30 ms dead time, ``delta=0.07``, in frames of ``sr / hop_length``).  ``normalize=True`` shifts and scales every row to
    [0, 1] in the envelope's precision, bit for bit as NumPy does; ``backtrack=True`` reads the normalised envelope (or ``energy``).  A
    normalised envelope without a non-zero entry, or with a non-finite one anywhere, gives no onsets: an empty array or an all-False one.

    Every argument is checked before any device work: ``y`` / ``onset_envelope``, ``units``, ``backtrack`` with ``sparse=False``, the rank
    with ``sparse=True``, ``hop_length``, the names in ``kwargs`` and the picker's ranges.  The reference checks ``units`` last, ``backtrack``
    and the picker's ranges only when the envelope has something to pick, and the rank inside the picker; so the two differ only where a call
    is wrong in one of these AND the envelope is empty of onsets: the reference returns the empty result, this raises.  An integer envelope
    with ``normalize=True`` raises ``TypeError`` as the reference's in-place division does; with ``normalize=False`` it is picked in float64,
    and a float16 envelope in float64 too.  The caller's arrays are never modified."""
    if onset_envelope is None and y is None:
        raise ParameterError("y or onset_envelope must be provided")
    src = onset_envelope if onset_envelope is not None else y
    if not is_torch_tensor(src):
        src = np.asarray(src)
    if sparse and units not in ("frames", "samples", "time"):
        raise ParameterError(f"Invalid unit type: {units}")
    if backtrack and not sparse:
        raise ParameterError("onset backtracking is only supported if sparse=True")
    if sparse and src.ndim != 1:  # from y the envelope's rank is y's rank
        raise ParameterError(f"sparse=True (default) does not support {src.ndim}-dimensional inputs. Either set sparse=False or process each dimension independently.")
    if src.ndim == 0:
        raise ParameterError("onset_detect needs an input of at least one dimension")
    if hop_length is None or not util.is_positive_int(hop_length):
        raise ParameterError(f"hop_length={hop_length} must be a positive integer")
    unknown = [k for k in kwargs if k not in _PICK_KEYS]
    if unknown:
        raise TypeError(f"peak_pick() got an unexpected keyword argument '{unknown[0]}'")
    kw = dict(kwargs)
    kw.setdefault("pre_max", 0.03 * sr // hop_length)  # 30ms (onset.py:184-189)
    kw.setdefault("post_max", 0.00 * sr // hop_length + 1)  # 0ms
    kw.setdefault("pre_avg", 0.10 * sr // hop_length)  # 100ms
    kw.setdefault("post_avg", 0.10 * sr // hop_length + 1)  # 100ms
    kw.setdefault("wait", 0.03 * sr // hop_length)  # 30ms
    kw.setdefault("delta", 0.07)
    params = _peaks.prepare(**kw)
    if backtrack and energy is not None:
        if not is_torch_tensor(energy):
            energy = np.asarray(energy)
        if energy.ndim != 1:
            raise ParameterError(f"energy must be one-dimensional, given energy.shape={tuple(energy.shape)}")
    job = dict(params=params, normalize=bool(normalize), backtrack=bool(backtrack), energy=energy if backtrack else None)

    if onset_envelope is not None:
        real = _peaks.row_dtype(src)
        if real is None and normalize:
            raise TypeError(f"Cannot cast ufunc 'divide' output from dtype('float64') to dtype('{_arrays.numpy_dtype_of(src)}') with casting rule 'same_kind'")
        got = _detect_given(src, real or np.dtype(np.float64), job)
    else:
        got = _detect_fused(src, sr, hop_length, job)
    lead = tuple(src.shape[:-1])
    n = int(src.shape[-1]) if onset_envelope is not None else 1 + int(src.shape[-1]) // int(hop_length)
    on_device = is_torch_tensor(src)
    if got is None:  # no onsets to grab (onset.py:176-180)
        if on_device:
            torch = _arrays._torch()
            onsets = torch.zeros(0, dtype=torch.int64, device=src.device) if sparse else torch.zeros(lead + (n,), dtype=torch.bool, device=src.device)
        else:
            onsets = np.array([], dtype=int) if sparse else np.zeros(lead + (n,), dtype=bool)
    else:
        rows, prev = got
        onsets = _peaks.to_bool(rows).reshape(lead + (n,))
        if sparse:
            onsets = _peaks.to_indices(onsets)
            if backtrack:
                onsets = _gather_minima(onsets, prev.reshape(-1))
    if not sparse:
        return onsets
    if on_device:
        if units == "samples":
            onsets = onsets * int(hop_length)
        elif units == "time":
            samples = (onsets * int(hop_length)).to(_arrays._torch().float64)
            onsets = samples / _arrays._torch().full_like(samples, float(sr))  # (a tensor divisor: a correctly rounded division, NumPy's bits; a scalar one is a multiplication by 1 / sr)
        return onsets
    if units == "samples":
        onsets = _convert.frames_to_samples(onsets, hop_length=hop_length)
    elif units == "time":
        onsets = _convert.frames_to_time(onsets, hop_length=hop_length, sr=sr)
    return onsets


def _gather_minima(events, prev):
    """``minima[match_events(events, minima, right=False)]`` from the row of preceding minima: events past the end take the last minimum;
    an empty event list and a negative event raise as ``util.match_events`` does (``util/matching.py:279-305``)."""
    if int(events.shape[0]) == 0:
        raise ParameterError("Attempting to match empty event list")
    if int(events.min()) < 0:
        raise ParameterError("Cannot match events with right=False and min(events_to) > min(events_from)")
    m = int(prev.shape[0])
    if is_torch_tensor(prev):
        torch = _arrays._torch()
        return prev[torch.clamp(events, max=m - 1)].to(torch.int64)
    return prev[np.minimum(events, m - 1)].astype(np.int64)


def _prev_minimum(sess, e_ptr, m, real):
    p_ptr, handle = sess.output((1, m), np.int32)
    sess.ctx.prev_minimum_exec(e_ptr, 1, m, real, p_ptr)
    return sess.result(handle)


def _detect_rows(sess, env_ptr, batch, n, real, job):
    """The picker (and the preceding minima) on a device envelope -> (handle of the uint8 rows, previous-minimum row or None, something to grab)."""
    own = job["backtrack"] and job["energy"] is None
    handle, norm_ptr, nonzero, finite = _peaks.pick_rows(sess, env_ptr, batch, n, real, job["params"], normalize=job["normalize"], keep_norm=own, status=True)
    prev = None
    if job["backtrack"] and nonzero and finite:
        if own:
            prev = _prev_minimum(sess, norm_ptr, n, real)
        else:
            energy = job["energy"]
            e_real = _peaks.row_dtype(energy) or np.dtype(np.float64)
            e = energy if is_torch_tensor(energy) and sess.is_torch else _spectrum._as_like(sess, energy.detach().cpu().numpy() if is_torch_tensor(energy) else energy)
            m = int(energy.shape[0])
            if m == 0:
                raise ParameterError("energy must not be empty")
            prev = _prev_minimum(sess, sess.input_raw(e, e_real), m, e_real)
    return handle, prev, bool(nonzero and finite)


def _detect_given(env, real, job):
    on_device = is_torch_tensor(env)
    lead, n = tuple(env.shape[:-1]), int(env.shape[-1])
    batch = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if n == 0 or batch == 0:
        return None
    if not on_device:
        # onset.py:164-176 on the host: an envelope with nothing to grab needs no device (the device repeats the arithmetic bit for bit)
        e = env.astype(real, copy=False)
        if job["normalize"]:
            e = e - np.min(e, keepdims=True, axis=-1)
            e /= np.max(e, keepdims=True, axis=-1) + util.tiny(e)
        if not e.any() or not np.all(np.isfinite(e)):
            return None
    sess = _arrays.Session(env if on_device else np.empty(0))
    try:
        env_ptr = sess.input_raw(env.reshape(batch, n), real)
        handle, prev, alive = _detect_rows(sess, env_ptr, batch, n, real, job)
        rows = sess.result(handle)
    finally:
        sess.close()
    return (rows, prev) if alive else None


def _detect_fused(y, sr, hop_length, job):
    side = {}

    def stage(sess, env_ptr, rows, n_env, real):
        handle, side["prev"], side["alive"] = _detect_rows(sess, env_ptr, rows, n_env, real, job)
        return handle, 1, n_env

    rows = _strength_then(y, sr=sr, hop_length=hop_length, stage=stage)  # (..., 1, n)
    return (rows, side["prev"]) if side["alive"] else None


def onset_backtrack(events, energy):
    """Each event moved back to the nearest preceding local minimum of ``energy``; drop-in for ``librosa.onset.onset_backtrack``
    (``librosa/onset.py:370-441``).

    A minimum is frame 0, or a frame ``1 <= j <= len(energy) - 2`` with ``energy[j] <= energy[j - 1]`` and ``energy[j] < energy[j + 1]``.  The
    result has ``events.shape`` (``int64``; two events may share a minimum).  As in the reference: an event past the end takes the last
    minimum, ``len(energy) < 3`` sends every event to 0, and an empty event list or a negative event raises ``ParameterError``.  The minima
    are found on the device; a device tensor among the arguments gives a device tensor."""
    on_device = is_torch_tensor(events) or is_torch_tensor(energy)
    if not is_torch_tensor(events):
        events = np.asarray(events)
    if not is_torch_tensor(energy):
        energy = np.asarray(energy)
    if energy.ndim != 1:
        raise ParameterError(f"energy must be one-dimensional, given energy.shape={tuple(energy.shape)}")
    shape = tuple(events.shape)
    flat = events.reshape(-1)
    if int(flat.shape[0]) == 0:
        raise ParameterError("Attempting to match empty event list")
    if _arrays.numpy_dtype_of(flat).kind == "f":
        flat = flat.floor().to(_arrays._torch().int64) if is_torch_tensor(flat) else np.floor(flat).astype(np.int64)
    if int(flat.min()) < 0:
        raise ParameterError("Cannot match events with right=False and min(events_to) > min(events_from)")
    m = int(energy.shape[0])
    like = energy if is_torch_tensor(energy) else events
    if m < 3:  # no interior frame: the only minimum is the padded 0
        if on_device:
            torch = _arrays._torch()
            return torch.zeros(shape, dtype=torch.int64, device=like.device)
        return np.zeros(shape, dtype=np.int64)
    real = _peaks.row_dtype(energy) or np.dtype(np.float64)
    sess = _arrays.Session(like if on_device else np.empty(0))
    try:
        if sess.is_torch and not is_torch_tensor(energy):
            energy = _spectrum._as_like(sess, energy)
        prev = _prev_minimum(sess, sess.input_raw(energy, real), m, real).reshape(-1)
    finally:
        sess.close()
    if is_torch_tensor(prev) and not is_torch_tensor(flat):
        flat = _arrays._torch().from_numpy(np.ascontiguousarray(flat, dtype=np.int64)).to(prev.device)
    return _gather_minima(flat, prev).reshape(shape)


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
