"""Beat tracking: ``beat_track`` with librosa's signature (``librosa/beat.py:89-317, 510-741``).

Onset strength with the median aggregate, the tempo estimate and Ellis's dynamic-programming tracker run on the device in one session.
From ``y``: the fused mel kernel, the per-clip maximum, the flux kernel (``aggregate=np.median``), the tempogram kernel in SUM mode with its
finishing launch, then the tracker's three launches (``csrc/lra_beat.h``: normalisation and frames per beat, the local score, and the
recurrence with the tail, the walk along the back-links and the trim), which read the BPM from device memory.  Only the BPM values and the
``uint8`` beat row come back.  ``sparse=True`` turns the row into indices (``np.flatnonzero``, or ``torch.nonzero`` for a device tensor).
Device tensors in give device tensors out.

Dtypes follow the reference: the normalised envelope and the local score have the envelope's precision (one rounding per term of the
convolution); the recurrence is float64 whatever the envelope is, with ``tightness`` rounded to float32 first.

Rows the reference cannot handle get no beats: a single-frame envelope (the reference raises ``IndexError`` inside ``localmax``), an
all-zero row beside live rows (its trim loop walks off the array), and a tempo whose ``round(sr / hop_length * 60 / bpm)`` is below 2 frames
(its search then reads a score it has not computed yet).
"""
from __future__ import annotations

import numpy as np

from . import _arrays, onset
from .core import convert
from .core import spectrum as _spectrum
from .feature import rhythm as _rhythm
from .util import utils as util
from .util.exceptions import ParameterError
from .util.utils import is_torch_tensor

__all__ = ["beat_track"]

# bpm modes of lra_beat_exec (include/librosa_amd.h)
_PER_ROW, _PER_FRAME = 0, 1


def beat_track(*, y=None, sr=22050, onset_envelope=None, hop_length=512, start_bpm=120.0, tightness=100, trim=True, bpm=None, prior=None, units="frames", sparse=True):
    """Dynamic-programming beat tracker; drop-in for ``librosa.beat.beat_track`` (``librosa/beat.py:89-317``).

    Returns ``(tempo, beats)``.  ``bpm=None``: the tempo is ``feature.tempo(onset_envelope=..., sr, hop_length, start_bpm, prior)``, shape
    ``(..., 1)``; a given ``bpm`` (a scalar, one value per channel, or one value per frame) is returned unchanged.  ``sparse=True``
    (one-dimensional input only): ``beats`` are ``int64`` frame indices, or samples / seconds with ``units``; ``sparse=False``: a bool array of
    the envelope's shape.  An envelope without a non-zero entry gives ``(0.0, [])``, or zeros of the leading shape and an all-False array.

    Every argument is checked before any device work.  The reference checks ``units`` and ``tightness`` after the tracker ran, so the two
    differ only for an all-zero envelope with bad ``units`` / ``tightness``: the reference returns the empty result, this raises."""
    if onset_envelope is None and y is None:
        raise ParameterError("y or onset_envelope must be provided")
    src = onset_envelope if onset_envelope is not None else y
    if not is_torch_tensor(src):
        src = np.asarray(src)
        if onset_envelope is not None:
            onset_envelope = src
        else:
            y = src
    ndim = src.ndim  # from y the envelope's rank is y's rank
    if sparse and ndim != 1:
        raise ParameterError(f"sparse=True (default) does not support {ndim}-dimensional inputs. Either set sparse=False or convert the signal to mono.")
    if sparse and units not in ("frames", "samples", "time"):
        raise ParameterError(f"Invalid unit type: {units}")
    if tightness <= 0:
        raise ParameterError("tightness must be strictly positive")
    if hop_length is None or not util.is_positive_int(hop_length):
        raise ParameterError(f"hop_length={hop_length} must be a positive integer")
    lead = tuple(src.shape[:-1])
    n = int(src.shape[-1]) if onset_envelope is not None else 1 + int(src.shape[-1]) // int(hop_length)
    bpm_rows, mode = None, _PER_ROW
    if bpm is not None:
        bpm_rows, mode = _expand_bpm(bpm, ndim, lead, n)
    job = None
    if bpm is None:
        # feature.tempo at its defaults (std_bpm=1, ac_size=8, max_tempo=320, aggregate=np.mean)
        job = _rhythm._tempo_job(_rhythm._ac_frames(8.0, sr, hop_length), sr, hop_length, start_bpm, 1.0, 320.0, prior, _rhythm._SUM)
        _rhythm._check_length(n, job)
    frame_rate = float(sr) / hop_length

    if onset_envelope is not None:
        got = _given(onset_envelope, lead, n, bpm_rows, mode, job, frame_rate, tightness, trim)
    else:
        got = _fused(y, sr, hop_length, lead, n, bpm_rows, mode, job, frame_rate, tightness, trim)
    if got is None:  # no onsets to grab (beat.py:279-285)
        if sparse:
            return 0.0, (_arrays._torch().zeros(0, dtype=_arrays._torch().int64, device=src.device) if is_torch_tensor(src) else np.array([], dtype=int))
        if is_torch_tensor(src):
            torch = _arrays._torch()
            return torch.zeros(lead, dtype=torch.float64, device=src.device), torch.zeros(lead + (n,), dtype=torch.bool, device=src.device)
        return np.zeros(shape=lead, dtype=float), np.zeros(lead + (n,), dtype=bool)
    tempo, beats = got
    if bpm is not None:
        tempo = bpm
    if is_torch_tensor(beats):
        beats = beats != 0
    else:
        beats = beats.astype(bool)
    if not sparse:
        return tempo, beats
    if is_torch_tensor(beats):
        torch = _arrays._torch()
        idx = torch.nonzero(beats).reshape(-1)
        if units == "samples":
            idx = idx * int(hop_length)
        elif units == "time":
            idx = (idx * int(hop_length)).to(torch.float64) / float(sr)
        return tempo, idx
    idx = np.flatnonzero(beats)
    if units == "samples":
        idx = convert.frames_to_samples(idx, hop_length=hop_length)
    elif units == "time":
        idx = convert.frames_to_time(idx, hop_length=hop_length, sr=sr)
    return tempo, idx


def _expand_bpm(bpm, ndim, lead, n):
    """beat.py:298-301 and :533-542: ``util.expand_to`` over the leading axes, the checks, and one float64 row (or value) per envelope."""
    b = bpm.detach().cpu().numpy() if is_torch_tensor(bpm) else bpm
    b = np.atleast_1d(b)
    if b.ndim > ndim:
        raise ParameterError(f"Cannot expand bpm of shape={b.shape} to fewer dimensions ndim={ndim}")
    b = b.reshape(tuple(b.shape) + (1,) * (ndim - b.ndim))
    if np.any(b <= 0):
        raise ParameterError(f"bpm={bpm} must be strictly positive")
    if b.shape[-1] not in (1, n):
        raise ParameterError(f"Invalid bpm shape={b.shape} does not match onset envelope shape={lead + (n,)}")
    try:
        b = np.broadcast_to(b, lead + (b.shape[-1],))
    except ValueError:
        raise ParameterError(f"Invalid bpm shape={b.shape} does not match onset envelope shape={lead + (n,)}") from None
    mode = _PER_FRAME if b.shape[-1] == n and n != 1 else _PER_ROW
    return np.ascontiguousarray(b, dtype=np.float64).reshape(-1, b.shape[-1]), mode


def _handle_ptr(sess, handle):
    return handle.data_ptr() if sess.is_torch else handle[0].ptr


def _track(sess, env_ptr, batch, n, real, bpm_rows, mode, job, frame_rate, tightness, trim):
    """Tempo (unless given) and the tracker on a device envelope -> (tempo handle or None, beat handle, any non-zero entry)."""
    ctx = sess.ctx
    tempo_handle = None
    if bpm_rows is None:
        tempo_handle, _, _ = _rhythm._device(sess, env_ptr, batch, n, real, job)
        bpm_ptr = _handle_ptr(sess, tempo_handle)
    else:
        bpm_ptr = sess.input_raw(_spectrum._as_like(sess, bpm_rows), np.float64)
    out_ptr, handle = sess.output((batch, n), np.uint8)
    work_ptr = sess.scratch(ctx.beat_work_bytes(batch, n, mode))
    alive = ctx.beat_exec(env_ptr, batch, n, real, bpm_ptr, mode, frame_rate, tightness, trim, out_ptr, work_ptr)
    return tempo_handle, handle, alive


def _given(env, lead, n, bpm_rows, mode, job, frame_rate, tightness, trim):
    on_device = is_torch_tensor(env)
    if n == 0 or (not on_device and not env.any()):
        return None
    real = np.dtype(np.float32) if _arrays.numpy_dtype_of(env) == np.float32 else np.dtype(np.float64)
    batch = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if batch == 0:
        return None
    sess = _arrays.Session(env if on_device else np.empty(0))
    try:
        env_ptr = sess.input_raw(env.reshape(batch, n), real)
        tempo_handle, handle, alive = _track(sess, env_ptr, batch, n, real, bpm_rows, mode, job, frame_rate, tightness, trim)
        beats = sess.result(handle)
        tempo = sess.result(tempo_handle) if tempo_handle is not None else None
    finally:
        sess.close()
    if not alive:
        return None
    return (tempo.reshape(lead + (1,)) if tempo is not None else None), beats.reshape(lead + (n,))


def _fused(y, sr, hop_length, lead, n, bpm_rows, mode, job, frame_rate, tightness, trim):
    side = {}

    def stage(sess, env_ptr, rows, n_env, real):
        tempo_handle, handle, alive = _track(sess, env_ptr, rows, n_env, real, bpm_rows, mode, job, frame_rate, tightness, trim)
        side["alive"] = alive
        side["tempo"] = sess.result(tempo_handle) if tempo_handle is not None else None
        return handle, 1, n_env

    beats = onset._strength_then(y, sr=sr, hop_length=hop_length, stage=stage, aggregate=np.median)  # (..., 1, n)
    if not side["alive"]:
        return None
    tempo = side["tempo"]
    return (tempo.reshape(lead + (1,)) if tempo is not None else None), beats.reshape(lead + (n,))
