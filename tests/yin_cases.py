"""Cases, inputs and the NumPy model of ``yin`` shared by ``scripts/make_yin_golden.py``, ``tests/test_yin_host.py`` and
``tests/test_yin_gpu.py``.

TEST INFRASTRUCTURE ONLY.  Inputs come from seeds and last 0.06 to 0.5 s (most 0.1 to 0.15 s): shorter than the 0.3 to 0.5 s the families
were first meant to have, because the golden file stores a dense CMND per case and has to stay under 1 MiB; the frame counts still cover 1, 15,
16, 17 and several workgroups.  Further down: ``tests/golden/yin.npz`` holds the unmodified reference's ``f0`` and cumulative mean
normalised difference function (CMND), digests of the inputs, exception names, warning texts and the measured error figures below.  The model
follows ``librosa/core/pitch.py:369-628`` line by line in the dtype it is handed (hand it float64 samples for the float64 model).

The selection is discrete (the first trough below the threshold, else the first minimum), so a comparison closer than the arithmetic's noise
may fall either way.  A frame is SETTLED when every comparison that decides its lag holds by more than ``eps`` on the float64 model, with
``eps`` = 4 times the largest difference between the reference's float32 and float64 CMND of the case's samples (stored by the generator; the
factor 4 is slack over the float32 run's own worst error).  At most 10 % of a case's non-silent frames and 3 % over all cases may be unsettled;
on failure the signal or seed is changed, not the bars.  All-zero frames are exact: ``f0 = sr / min_period``.

Bounds on settled frames.  ``f0`` against the float64 model: 16 times the largest relative distance between the reference's float64 ``f0`` and
a ``np.longdouble`` evaluation of the cancellation-free difference function, per case (stored), at least 4 float64 ulp; the factor 16 allows
for a transform of other length and radices and for fused multiply-adds.  For float32 samples the device is also no further from that model
than twice the reference's own float32 run.  The dense CMND has the same two rules with its own stored figure (``ref_cmnd_err``, relative to
max(1, |c|)), plus one rounding to the input's type.  A parabolic shift ``-b / a`` moves by at most ``5 delta / |a|`` when every CMND value moves
by ``delta`` (``|db| <= delta``, ``|da| <= 4 delta``, ``|shift| < 1``), and only where ``| |b| - |a| | > 5 delta`` is its ``|b| >= |a|`` test decided.
"""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "yin.npz")
SR = 22050
FRAME_RUN = 16                # frames per workgroup (csrc/lra_yin.h: kYinGroup)
EPS_FACTOR, F0_FACTOR, F0_FLOOR_ULP = 4.0, 16.0, 4.0
MAX_UNSETTLED_CASE, MAX_UNSETTLED_ALL = 0.10, 0.03
# the transform lengths the device library is compiled for (csrc/lra_mixed_sizes.h: LRA_MIXED_SIZES)
SIZES = (160, 200, 240, 320, 400, 480, 600, 640, 720, 800, 882, 960, 1000, 1200, 1280, 1440, 1600, 1764, 1920, 2000, 2400, 2646, 3200, 3528, 4800)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
# name -> dict(kind, n, lead, dtype, seed, kw (yin's keyword arguments))
CASES = {}


def _add(name, kind, n, *, lead=(), dtype="float32", **kw):
    kw.setdefault("sr", SR)
    CASES[name] = dict(kind=kind, n=int(n), lead=tuple(lead), dtype=dtype, seed=7000 + len(CASES), kw=kw)


W64 = dict(fmin=800.0, fmax=8000.0, frame_length=64, hop_length=16)          # 27 lags, transform 160
W512 = dict(fmin=100.0, fmax=2000.0, frame_length=512, hop_length=128)       # transform 800, two frames per chunk
W1001 = dict(fmin=80.0, fmax=1500.0, frame_length=1001, hop_length=300)      # odd, the hop does not divide it; transform 1280
W2048 = dict(fmin=65.0, fmax=2093.0, frame_length=2048)                      # the defaults; transform 2400 (the reference pads to 4096)
W4500 = dict(fmin=65.0, fmax=2093.0, frame_length=4500, hop_length=2048)     # 4500 + 340 > 4800: the direct kernel
for _kind in ("glide", "noise", "gap", "zeros"):
    _add(f"w512_{_kind}", _kind, 0.15 * SR, **W512)
_add("w512_glide64", "glide", 0.15 * SR, dtype="float64", **W512)
_add("w512_gap64", "gap", 0.15 * SR, dtype="float64", **W512)
_add("w64_glide", "glide_hi", 0.1 * SR, **W64)
_add("w64_noise64", "noise", 0.1 * SR, dtype="float64", **W64)
_add("w1001_glide", "glide", 0.3 * SR, **W1001)
_add("w1001_gap64", "gap", 0.3 * SR, dtype="float64", **W1001)
_add("w2048_glide", "glide", 0.5 * SR, **W2048)
_add("w2048_noise64", "noise", 0.3 * SR, dtype="float64", **W2048)
_add("w4500_glide", "glide", 0.5 * SR, **W4500)
_add("w4500_gap64", "gap", 0.5 * SR, dtype="float64", **W4500)
# 1 frame, and one frame below, at and above a workgroup's run (centred: 1 + n // hop frames)
for _frames in (1, FRAME_RUN - 1, FRAME_RUN, FRAME_RUN + 1):
    _add(f"frames{_frames}", "glide_hi", (_frames - 1) * 32 + 20, fmin=800.0, fmax=8000.0, frame_length=64, hop_length=32)
for _lead in ((2,), (2, 3)):
    _add(f"lead{len(_lead)}", "glide", 0.06 * SR, lead=_lead, **W512)
    _add(f"lead{len(_lead)}_64", "noise", 0.06 * SR, lead=_lead, dtype="float64", **W512)
_add("nocenter", "glide", 0.15 * SR, center=False, **W512)
_add("nocenter_one", "glide", 512, center=False, **W512)  # exactly one frame
_add("reflect", "glide", 0.12 * SR, pad_mode="reflect", **W512)
_add("edge64", "glide", 0.12 * SR, pad_mode="edge", dtype="float64", **W512)
_add("symmetric", "glide", 0.12 * SR, pad_mode="symmetric", **W1001)
_add("linear_ramp64", "glide", 0.12 * SR, pad_mode="linear_ramp", dtype="float64", **W512)  # padded on the host (float64: np.pad rounds the ramp to the samples' type)
_add("nyquist", "glide_hi", 0.1 * SR, fmin=800.0, fmax=SR / 2, frame_length=64, hop_length=16)  # min_period = 2
_add("thr0", "glide", 0.15 * SR, trough_threshold=0.0, **W512)  # always the fallback
_add("thr1", "glide", 0.15 * SR, trough_threshold=1.0, **W512)
_add("thr1_noise", "noise", 0.15 * SR, trough_threshold=1.0, **W512)
# a sine of exactly min_period = 10 samples: chosen at lag index 0 by the first-lag rule
_add("first_lag", "sine10", 0.1 * SR, fmin=441.0, fmax=2205.0, frame_length=512, hop_length=128)
# a sine of 52 samples, two more than max_period = 50, and no threshold: the CMND still falls at the last lag, which the fallback picks; the shift is 0 there
_add("last_lag", "sine52", 0.1 * SR, trough_threshold=0.0, fmin=441.0, fmax=2205.0, frame_length=512, hop_length=128)
_add("two_periods_warning", "glide", 0.12 * SR, fmin=65.0, fmax=2093.0, frame_length=512, hop_length=128)  # sr / fmin >= frame_length // 2
# more than 64 KiB of LDS, which a launch has to ask for: the 4800-point transform (2048 + 2005 lags, one frame per chunk, about 93 KB) ...
_add("w2048_fmin11", "glide", 0.1 * SR, fmin=11.0, fmax=2093.0, frame_length=2048, hop_length=512)
# ... and the direct kernel with 4410 lags (about 70 KB)
_add("w8192_fmin5", "glide", 0.4 * SR, fmin=5.0, fmax=2093.0, frame_length=8192, hop_length=4096)

ERRORS = {
    "no_fmin": dict(fmin=None, fmax=2000.0),
    "no_fmax": dict(fmin=100.0, fmax=None),
    "fmax_above_nyquist": dict(fmin=100.0, fmax=SR / 2 + 1),
    "fmin_not_below_fmax": dict(fmin=500.0, fmax=500.0),
    "fmin_not_positive": dict(fmin=0.0, fmax=2000.0),
    "fmin_too_small": dict(fmin=10.0, fmax=2000.0, frame_length=512),
    "too_short": dict(fmin=100.0, fmax=2000.0, frame_length=512, center=False, n=300),
    "bad_hop": dict(fmin=100.0, fmax=2000.0, frame_length=512, hop_length=0),
    "integer_audio": dict(fmin=100.0, fmax=2000.0, dtype="int16"),
    "not_finite": dict(fmin=100.0, fmax=2000.0, nan=True),
}


def error_call(name):
    """(y, kwargs) of an ERRORS entry."""
    kw = dict(ERRORS[name])
    y = np.ones(int(kw.pop("n", 4096)), dtype=kw.pop("dtype", "float32"))
    if kw.pop("nan", False):
        y[17] = np.nan
    return y, dict(sr=SR, **kw)


def signal(name):
    """The (..., n) samples of a case, in its dtype."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    n, sr = c["n"], c["kw"]["sr"]
    shape = c["lead"] + (n,)
    t = np.arange(n) / sr
    kind = c["kind"]
    if kind in ("glide", "glide_hi"):
        f_lo, f_hi = (180.0, 420.0) if kind == "glide" else (1000.0, 2600.0)
        lo = f_lo * (1.0 + 0.2 * rng.random(c["lead"] + (1,)))
        phase = 2 * np.pi * (lo * t + 0.5 * (f_hi - f_lo) / max(t[-1], 1.0 / sr) * t * t)
        y = np.sin(phase) + 0.5 * np.sin(2 * phase + 0.3) + 0.25 * np.sin(3 * phase + 1.1) + 0.01 * rng.standard_normal(shape)
        y *= 0.4
    elif kind == "noise":
        y = 0.3 * rng.standard_normal(shape)
    elif kind == "gap":
        y = 0.5 * np.sin(2 * np.pi * 331.0 * t + 0.2) + 0.2 * np.sin(2 * np.pi * 662.0 * t) + 0.005 * rng.standard_normal(shape)
        y[..., n // 3 : n // 3 + n // 3] = 0.0
    elif kind == "zeros":
        y = np.zeros(shape)
    elif kind in ("sine10", "sine52"):
        period = 10 if kind == "sine10" else 52
        y = 0.5 * np.sin(2 * np.pi * np.arange(n) / period + 0.4) + np.zeros(shape)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(y.astype(c["dtype"]))


def periods(kw):
    sr, W = kw["sr"], kw.get("frame_length", 2048)
    return int(np.floor(sr / kw["fmax"])), min(int(np.ceil(sr / kw["fmin"])), W - 1)


def transform_length(W, P):
    """csrc/lra_yin_launch.h: the smallest compiled size of at least W + P points, 0 for the direct kernel."""
    fit = [s for s in SIZES if s >= W + P]
    return min(fit) if fit else 0


def chunk_frames(N):
    """csrc/lra_yin.h: chunk_frames_of."""
    fc = FRAME_RUN
    while fc > 1 and fc * 2 * (N // 2) * 16 > 48 * 1024:
        fc //= 2
    return fc


# ---- the model, line by line --------------------------------------------------------------------------------------------------------------------
def frame(y, frame_length, hop_length):
    """util.frame(y, frame_length=, hop_length=) on the last axis: (..., frame_length, n_frames)."""
    n_frames = 1 + (y.shape[-1] - frame_length) // hop_length
    idx = np.arange(frame_length)[:, None] + hop_length * np.arange(n_frames)[None, :]
    return y[..., idx]


def framed(y, *, frame_length=2048, hop_length=None, center=True, pad_mode="constant", **_):
    if hop_length is None:
        hop_length = frame_length // 4
    if center:
        padding = [(0, 0)] * y.ndim
        padding[-1] = (frame_length // 2, frame_length // 2)
        y = np.pad(y, padding, mode=pad_mode)
    return frame(y, frame_length, hop_length)


def autocorrelate(y, max_size):
    """core/audio.py:1320-1394 along axis -2."""
    import scipy.fft

    n_pad = scipy.fft.next_fast_len(2 * y.shape[-2] - 1, real=True)
    spec = scipy.fft.rfft(y, n=n_pad, axis=-2)
    powspec = spec.real**2 + spec.imag**2
    return scipy.fft.irfft(powspec, n=n_pad, axis=-2)[..., :max_size, :]


def tiny(x):
    return np.finfo(x.dtype if np.issubdtype(x.dtype, np.floating) else np.float32).tiny


def model_cmnd(y_frames, min_period, max_period):
    """_cumulative_mean_normalized_difference (core/pitch.py:369-418)."""
    acf_frames = autocorrelate(y_frames, max_period + 1)
    yin_frames = np.square(y_frames)
    np.cumsum(yin_frames, out=yin_frames, axis=-2)
    k = slice(1, max_period + 1)
    yin_frames[..., 0, :] = 0
    yin_frames[..., k, :] = 2 * (acf_frames[..., 0:1, :] - acf_frames[..., k, :]) - yin_frames[..., : k.stop - 1, :]
    return _normalise(yin_frames, min_period, max_period)


def _normalise(yin_frames, min_period, max_period):
    k = slice(1, max_period + 1)
    yin_numerator = yin_frames[..., min_period : max_period + 1, :]
    k_range = np.r_[k].reshape((-1, 1))
    cumulative_mean = np.cumsum(yin_frames[..., k, :], axis=-2) / k_range
    yin_denominator = cumulative_mean[..., min_period - 1 : max_period, :]
    return yin_numerator / (yin_denominator + tiny(yin_denominator))


def exact_cmnd(y_frames, min_period, max_period):
    """The cancellation-free difference function in np.longdouble: d(k) = sum_{j < W - k} (y_j - y_{j + k})^2 + sum_{j >= W - k} y_j^2, and
    y_0^2 more at k = 1 (the reference reads E(0) as 0)."""
    y = y_frames.astype(np.longdouble)
    W = y.shape[-2]
    d = np.zeros(y.shape[:-2] + (max_period + 1, y.shape[-1]), dtype=np.longdouble)
    sq = y * y
    for k in range(1, max_period + 1):
        diff = y[..., : W - k, :] - y[..., k:, :]
        d[..., k, :] = (diff * diff).sum(axis=-2) + sq[..., W - k :, :].sum(axis=-2)
    d[..., 1, :] += sq[..., 0, :]
    return _normalise(d, min_period, max_period)


def parabolic_shifts(x):
    """_parabolic_interpolation along axis -2 (core/pitch.py:421-477)."""
    shifts = np.zeros_like(x)
    a = x[..., 2:, :] + x[..., :-2, :] - 2 * x[..., 1:-1, :]
    b = (x[..., 2:, :] - x[..., :-2, :]) / 2
    with np.errstate(all="ignore"):
        shifts[..., 1:-1, :] = np.where(np.abs(b) >= np.abs(a), 0, -b / np.where(a == 0, 1, a))
    return shifts


def localmin(x):
    """util.localmin along axis -2 (util/utils.py:1121-1180): the first element never, the last on the first test alone."""
    out = np.zeros(x.shape, dtype=bool)
    out[..., 1:-1, :] = (x[..., 1:-1, :] < x[..., :-2, :]) & (x[..., 1:-1, :] <= x[..., 2:, :])
    out[..., -1, :] = x[..., -1, :] < x[..., -2, :]
    return out


def select(yin_frames, min_period, trough_threshold, sr):
    """core/pitch.py:592-628 from the CMND on: (f0, lag index, parabolic shifts)."""
    shifts = parabolic_shifts(yin_frames)
    is_trough = localmin(yin_frames)
    is_trough[..., 0, :] = yin_frames[..., 0, :] < yin_frames[..., 1, :]
    is_threshold_trough = np.logical_and(is_trough, yin_frames < trough_threshold)
    global_min = np.argmin(yin_frames, axis=-2)[..., None, :]
    yin_period = np.argmax(is_threshold_trough, axis=-2)[..., None, :]
    none = np.all(~is_threshold_trough, axis=-2, keepdims=True)
    yin_period[none] = global_min[none]
    period = (min_period + yin_period + np.take_along_axis(shifts, yin_period, axis=-2))[..., 0, :]
    return sr / period, yin_period[..., 0, :], shifts


def model(y, *, fmin, fmax, sr=SR, frame_length=2048, hop_length=None, trough_threshold=0.1, center=True, pad_mode="constant", exact=False):
    """yin on (..., n) samples in y's dtype: dict(f0, index, cmnd, shifts, silent, min_period).  exact: the np.longdouble evaluation."""
    y_frames = framed(y, frame_length=frame_length, hop_length=hop_length, center=center, pad_mode=pad_mode)
    p0, p1 = periods(dict(sr=sr, fmin=fmin, fmax=fmax, frame_length=frame_length))
    cmnd = (exact_cmnd if exact else model_cmnd)(y_frames, p0, p1)
    f0, index, shifts = select(cmnd, p0, trough_threshold, sr)
    return dict(f0=f0, index=index, cmnd=cmnd, shifts=shifts, silent=~y_frames.any(axis=-2), min_period=p0)


# ---- settled frames ---------------------------------------------------------------------------------------------------------------------------
def settled(cmnd, trough_threshold, eps):
    """True per frame where the lag the float64 CMND selects (axis -2) is decided by margins above eps: every earlier lag is no trough below
    the threshold by more than eps, and the chosen one is (or, in the fallback, leads every other value by more than eps)."""
    c = np.moveaxis(np.asarray(cmnd, dtype=np.float64), -2, -1)  # (..., frames, lags)
    L = c.shape[-1]
    left = np.concatenate([np.full(c.shape[:-1] + (1,), np.inf), c[..., :-1]], axis=-1)   # no left neighbour at lag 0: that test is vacuous
    right = np.concatenate([c[..., 1:], np.full(c.shape[:-1] + (1,), np.inf)], axis=-1)   # and no right one at the last
    surely = (c < left - eps) & (c < right - eps) & (c < trough_threshold - eps)
    surely_not = (c > left + eps) | (c > right + eps) | (c > trough_threshold + eps)
    first = np.argmax(surely, axis=-1)
    lags = np.arange(L)
    before_ok = np.all(surely_not | (lags >= first[..., None]), axis=-1)
    by_threshold = surely.any(axis=-1) & before_ok
    order = np.sort(c, axis=-1)
    by_fallback = surely_not.all(axis=-1) & (order[..., 1] - order[..., 0] > eps)
    return by_threshold | by_fallback


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return np.abs(a - b) / np.abs(b)


def cmnd_err(a, b):
    """|a - b| relative to max(1, |b|): the CMND is O(1) on a live frame and 0 on a silent one."""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return np.abs(a - b) / np.maximum(1, np.abs(b))


def cmnd_bound(meta_case):
    """The device's bound on the CMND against the float64 model, as f0_bound."""
    return max(F0_FACTOR * meta_case["ref_cmnd_err"], F0_FLOOR_ULP * np.finfo(np.float64).eps)


def f0_bound(meta_case):
    """The device's bound on settled frames against the float64 model (relative)."""
    return max(F0_FACTOR * meta_case["ref_f0_err"], F0_FLOOR_ULP * np.finfo(np.float64).eps)


_models = {}


def model64(name):
    """The float64 model of a case's samples, computed once and left unchanged."""
    if name not in _models:
        _models[name] = model(signal(name).astype(np.float64), **CASES[name]["kw"])
    return _models[name]


def settled_frames(name, meta):
    m = model64(name)
    return settled(m["cmnd"], CASES[name]["kw"].get("trough_threshold", 0.1), meta["cases"][name]["eps"]) & ~m["silent"]


def check_f0(got, name, z, meta):
    """What the simulator and the device owe on a case: silent frames exact; on settled frames the reference's lag, f0 within f0_bound of the
    float64 model and, for float32 samples, within twice the reference's own float32 distance.  Returns the worst relative error."""
    kw, m, want = CASES[name]["kw"], model64(name), z["f0_" + name]
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.all(got[m["silent"]] == kw["sr"] / m["min_period"])
    ok = settled_frames(name, meta)
    err = np.max(rel_err(got[ok], m["f0"][ok]), initial=0)
    print(f"{name}: f0 err {float(err):.3e} bound {f0_bound(meta['cases'][name]):.3e}")
    lag = np.rint(kw["sr"] / got - m["min_period"] - np.take_along_axis(m["shifts"], m["index"][..., None, :], axis=-2)[..., 0, :])
    assert np.array_equal(lag[ok], m["index"][ok]), "another lag than the reference's on a settled frame"
    assert err <= f0_bound(meta["cases"][name])
    if CASES[name]["dtype"] == "float32":
        own = np.max(rel_err(want[ok], m["f0"][ok]), initial=0)
        assert err <= 2 * own
    return float(err)


def check_frames(cm, sh, m, want, meta_case, dtype):
    """The two rules of f0 on the dense CMND, and the shifts within what the CMND's bound allows (tests/yin_cases.py)."""
    rounding = np.finfo(np.float32).eps / 2 if dtype == np.float32 else 0.0  # computed in float64, rounded once to the input's type
    bound = cmnd_bound(meta_case)
    err = float(np.max(cmnd_err(cm, m["cmnd"])))
    print(f"cmnd err {err:.3e} bound {bound + rounding:.3e}")
    assert err <= bound + rounding
    if dtype == np.float32:  # no further from the model than twice the reference's own float32 run
        assert np.max(np.abs(cm - m["cmnd"])) <= 2 * np.max(np.abs(want - m["cmnd"]))
    silent = np.broadcast_to(m["silent"][..., None, :], cm.shape)
    assert not cm[silent].any() and not sh[silent].any()
    assert not sh[..., 0, :].any() and not sh[..., -1, :].any() and np.all(np.abs(sh) < 1)
    c = m["cmnd"]
    a, b = c[..., 2:, :] + c[..., :-2, :] - 2 * c[..., 1:-1, :], (c[..., 2:, :] - c[..., :-2, :]) / 2
    delta = bound * np.maximum(1.0, np.max(np.abs(c)))
    firm = np.abs(np.abs(b) - np.abs(a)) > 5 * delta
    assert firm[~silent[..., 1:-1, :]].mean() > 0.9  # (a silent frame has a = b = 0: its shifts are 0 by the test above)
    with np.errstate(all="ignore"):
        allowed = 5 * delta / np.abs(a) + rounding
    excess = (np.abs(sh[..., 1:-1, :] - m["shifts"][..., 1:-1, :]) - allowed)[firm]
    assert np.max(excess, initial=-1.0) <= 0


def load():
    z = np.load(GOLDEN)
    return z, json.loads(bytes(z["meta"]).decode())
