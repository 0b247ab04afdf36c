"""Rhythm features: ``tempogram``, ``fourier_tempogram`` and ``tempo`` with librosa's signatures (``librosa/feature/rhythm.py:38-471``).

The autocorrelation tempogram runs in one launch (``csrc/lra_rhythm.h``): every frame of the (linear-ramp padded) onset envelope is
windowed and autocorrelated in float64 through a real FFT of a length from the mixed-radix list (>= 2 win_length - 1), and each column is
normalised (``norm`` in ``np.inf`` / ``None`` / ``1`` / ``2``).  The result is float64 whatever the envelope's precision, as in the reference.
``tempo`` runs the same kernel with the scoring folded in: ``aggregate=np.mean`` sums the normalised columns per group of frames and a
second small launch adds the groups in a fixed order, divides by the frame count and takes the prior-weighted argmax;
``aggregate=None`` scores every frame in the kernel.  Only the BPM values are downloaded.  From ``y`` the onset envelope never leaves the
device (``onset._strength_then``: onset's three launches, then the tempogram's one or two).

Slow paths, on the host over a downloaded array: any other ``norm`` (``util.normalize`` applied to the device's unnormalised
autocorrelation), any other ``aggregate`` callable, and a given ``tg`` (the scoring only).  The BPM and log-prior tables are always built on
the host with the reference's own NumPy expressions.  Device tensors in give device tensors out.
"""
from __future__ import annotations

import numpy as np

from .. import _arrays, filters, onset
from ..core import convert
from ..core import spectrum as _spectrum
from ..util import utils as util
from ..util.exceptions import ParameterError
from ..util.utils import is_torch_tensor

__all__ = ["tempogram", "fourier_tempogram", "tempo"]

# modes and norm codes of lra_tempogram_exec (include/librosa_amd.h)
_WRITE, _SUM, _ARGMAX = 0, 1, 2
_NORM_NONE, _NORM_INF, _NORM_L1, _NORM_L2 = 0, 1, 2, 3


def tempogram(*, y=None, sr=22050, onset_envelope=None, hop_length=512, win_length=384, center=True, window="hann", norm=np.inf):
    """Autocorrelation tempogram; drop-in for ``librosa.feature.tempogram`` (``librosa/feature/rhythm.py:38-191``).

    Returns float64 ``(..., win_length, n_frames)``.  ``onset_envelope`` takes precedence over ``y``; without it the envelope is
    ``onset.onset_strength(y=y, sr=sr, hop_length=hop_length)``, computed and consumed on the device."""
    if win_length < 1:
        raise ParameterError("win_length must be a positive integer")
    win_length = int(win_length)
    ac_window = np.ascontiguousarray(filters.get_window(window, win_length, fftbins=True), dtype=np.float64)
    code = _norm_code(norm)
    job = dict(W=win_length, center=bool(center), window=ac_window, norm=_NORM_NONE if code is None else code, mode=_WRITE)
    res = _run(y, sr, onset_envelope, hop_length, job)
    if code is None:
        # slow path: util.normalize on the host over the unnormalised autocorrelation (finiteness was checked on the device)
        host = res.detach().cpu().numpy() if is_torch_tensor(res) else res
        normed = util.normalize(host, norm=norm, axis=-2)
        return _arrays._torch().from_numpy(np.ascontiguousarray(normed)).to(res.device) if is_torch_tensor(res) else normed
    return res


def fourier_tempogram(*, y=None, sr=22050, onset_envelope=None, hop_length=512, win_length=384, center=True, window="hann"):
    """Fourier tempogram; drop-in for ``librosa.feature.fourier_tempogram`` (``librosa/feature/rhythm.py:194-292``): the short-time Fourier
    transform of the onset envelope with ``n_fft=win_length`` and ``hop_length=1``."""
    if win_length < 1:
        raise ParameterError("win_length must be a positive integer")
    if onset_envelope is None:
        if y is None:
            raise ParameterError("Either y or onset_envelope must be provided")
        onset_envelope = onset.onset_strength(y=y, sr=sr, hop_length=hop_length)
    return _spectrum.stft(onset_envelope, n_fft=win_length, hop_length=1, center=center, window=window)


def tempo(*, y=None, sr=22050, onset_envelope=None, tg=None, hop_length=512, start_bpm=120, std_bpm=1.0, ac_size=8.0, max_tempo=320.0, aggregate=np.mean, prior=None):
    """Tempo estimate in BPM; drop-in for ``librosa.feature.tempo`` (``librosa/feature/rhythm.py:295-471``).

    ``aggregate=np.mean`` gives ``(..., 1)``, ``aggregate=None`` a time-varying ``(..., n_frames)``; both run on the device.  Any other
    ``aggregate`` callable and a given ``tg`` take the host slow path (see the module docstring)."""
    if start_bpm <= 0:
        raise ParameterError("start_bpm must be strictly positive")
    if tg is None:
        win_length = _ac_frames(ac_size, sr, hop_length)
        device = aggregate is np.mean or aggregate is None
        if not device:
            tg = tempogram(y=y, sr=sr, onset_envelope=onset_envelope, hop_length=hop_length, win_length=win_length)
        else:
            job = _tempo_job(win_length, sr, hop_length, start_bpm, std_bpm, max_tempo, prior, _SUM if aggregate is np.mean else _ARGMAX)
            res = _run(y, sr, onset_envelope, hop_length, job)  # (..., 1, 1) or (..., 1, n_frames)
            return res[..., 0, :]
    else:
        win_length = int(tg.shape[-2])
    bpms, logprior = _tables(win_length, hop_length, sr, start_bpm, std_bpm, max_tempo, prior)
    return _score_host(tg, aggregate, bpms, logprior)


def _ac_frames(ac_size, sr, hop_length):
    """time_to_frames(ac_size, sr=sr, hop_length=hop_length) (core/convert.py: time_to_samples, samples_to_frames)."""
    return int(np.floor((np.asanyarray(ac_size) * sr).astype(int) // hop_length).astype(int))


def _tempo_job(win_length, sr, hop_length, start_bpm, std_bpm, max_tempo, prior, mode):
    """The tempogram kernel's job for a tempo estimate (``tempo`` and ``beat.beat_track`` share it): the tables, the Hann window, the mode."""
    if start_bpm <= 0:
        raise ParameterError("start_bpm must be strictly positive")
    if win_length < 1:
        raise ParameterError("win_length must be a positive integer")
    bpms, logprior = _tables(win_length, hop_length, sr, start_bpm, std_bpm, max_tempo, prior)
    ac_window = np.ascontiguousarray(filters.get_window("hann", win_length, fftbins=True), dtype=np.float64)
    return dict(W=win_length, center=True, window=ac_window, norm=_NORM_INF, mode=mode, bpms=bpms, logprior=logprior)


# ---- host tables and the slow path ------------------------------------------------------------------------------------------------------
def _tables(win_length, hop_length, sr, start_bpm, std_bpm, max_tempo, prior):
    """bpms and logprior exactly as the reference builds them (rhythm.py:445-463), float64."""
    bpms = convert.tempo_frequencies(win_length, hop_length=hop_length, sr=sr)
    if prior is None:
        logprior = -0.5 * ((np.log2(bpms) - np.log2(start_bpm)) / std_bpm) ** 2
    else:
        logprior = prior.logpdf(bpms)
    if max_tempo is not None:
        max_idx = int(np.argmax(bpms < max_tempo))
        logprior[:max_idx] = -np.inf
    return np.ascontiguousarray(bpms, dtype=np.float64), np.ascontiguousarray(logprior, dtype=np.float64)


def _score_host(tg, aggregate, bpms, logprior):
    """rhythm.py:441-471 on the host (a torch ``tg`` is downloaded, the estimate goes back to its device)."""
    dev = tg.device if is_torch_tensor(tg) else None
    host = tg.detach().cpu().numpy() if dev is not None else np.asarray(tg)
    if aggregate is not None:
        host = aggregate(host, axis=-1, keepdims=True)
    lp = logprior.reshape((1,) * (host.ndim - 2) + (-1, 1)) if host.ndim >= 2 else logprior
    best = np.argmax(np.log1p(1e6 * host) + lp, axis=-2)
    est = np.take(bpms, best)
    return _arrays._torch().from_numpy(np.ascontiguousarray(est)).to(dev) if dev is not None else est


def _norm_code(norm):
    """The device's norm code, or None: a norm for the host slow path."""
    if norm is None:
        return _NORM_NONE
    if isinstance(norm, (bool, np.bool_)) or not np.issubdtype(type(norm), np.number):
        return None
    if norm == np.inf:
        return _NORM_INF
    if norm == 1:
        return _NORM_L1
    if norm == 2:
        return _NORM_L2
    return None


def _check_length(n, job):
    """util.frame's check (after the centre padding), before any device work."""
    total = n + (2 * (job["W"] // 2) if job["center"] else 0)
    if total < job["W"]:
        raise ParameterError(f"Input is too short (n={total:d}) for frame_length={job['W']:d}")


# ---- device work ------------------------------------------------------------------------------------------------------------------------
def _run(y, sr, onset_envelope, hop_length, job):
    """The tempogram kernel on the given envelope or on onset_strength(y) -> (..., rows, cols): (W, n_frames) | (1, 1) | (1, n_frames)."""
    if onset_envelope is None:
        if y is None:
            raise ParameterError("Either y or onset_envelope must be provided")
        if hop_length is None or not util.is_positive_int(hop_length):
            raise ParameterError(f"hop_length={hop_length} must be a positive integer")
        _check_length(1 + int(y.shape[-1]) // int(hop_length), job)  # the centred mel's frame count = the envelope's

        def stage(sess, env_ptr, rows, n, real):
            return _device(sess, env_ptr, rows, n, real, job)

        return onset._strength_then(y, sr=sr, hop_length=hop_length, stage=stage)
    env = onset_envelope
    on_device = is_torch_tensor(env)
    if not on_device:
        env = np.asarray(env)
    real = np.dtype(np.float32) if _arrays.numpy_dtype_of(env) == np.float32 else np.dtype(np.float64)
    lead, n = tuple(env.shape[:-1]), int(env.shape[-1])
    _check_length(n, job)
    batch = int(np.prod(lead, dtype=np.int64)) if lead else 1
    sess = _arrays.Session(env if on_device else np.empty(0))
    try:
        env_ptr = sess.input_raw(env.reshape(batch, n), real)
        handle, rows, cols = _device(sess, env_ptr, batch, n, real, job)
        res = sess.result(handle)
    finally:
        sess.close()
    return res.reshape(lead + (rows, cols))


def _device(sess, env_ptr, batch, n, real, job):
    """lra_tempogram_exec on [batch][n] envelopes -> (handle, rows, cols)."""
    ctx = sess.ctx
    W, mode = job["W"], job["mode"]
    n_frames = n if job["center"] else n - W + 1
    win_ptr = sess.input_raw(_spectrum._as_like(sess, job["window"]), np.float64)
    lp_ptr = bp_ptr = None
    if mode != _WRITE:
        lp_ptr = sess.input_raw(_spectrum._as_like(sess, job["logprior"]), np.float64)
        bp_ptr = sess.input_raw(_spectrum._as_like(sess, job["bpms"]), np.float64)
    rows, cols = (W, n_frames) if mode == _WRITE else (1, 1 if mode == _SUM else n_frames)
    out_ptr, handle = sess.output((batch, rows, cols), np.float64)
    work_ptr = sess.scratch(ctx.tempogram_work_bytes(batch, n_frames, W, mode))
    if ctx.tempogram_exec(env_ptr, batch, n, real, W, job["center"], win_ptr, job["norm"], mode, lp_ptr, bp_ptr, out_ptr, work_ptr):
        raise ParameterError("Input must be finite")
    return handle, rows, cols
