"""The inputs and cases of tests/golden/peaks.npz, rebuilt from seeds (scripts/make_peak_golden.py stores only results, the reference's
envelopes and the inputs' checksums), and ``greedy_model``: the greedy picker written from its three documented conditions."""
import json
import os

import numpy as np

from beat_signals import FULL_ROWS, FULL_STORED, full_signal  # noqa: F401  (the full-size batch is beat_track's)
from rhythm_signals import SR
from rhythm_signals import make_inputs as _rhythm_inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "peaks.npz")

TILE, HALO, RING = 256, 64, 2048  # kTile, kHalo, kRing of csrc/lra_peaks.h (tests/test_peaks_host.py checks them against the header)
METHODS = ("greedy", "dp_count", "dp_value")

_W = dict(pre_max=3, post_max=3, pre_avg=3, post_avg=5, delta=0.3, wait=4)
_K16 = dict(sr=16000, hop_length=160)


def _w(**kw):
    return dict(_W, **kw)


# ---- util.peak_pick: name -> (input key, kwargs).  "r32_<n>_<seed>" / "r64_<n>_<seed>": |N(0, 1)| of that length and precision. --------
PICK = {}
for _n, _s in ((1, 1), (2, 2), (3, 3), (63, 4), (64, 5), (65, 6), (TILE - 1, 7), (TILE, 8), (TILE + 1, 9), (1292, 10)):
    PICK[f"greedy_f32_{_n}"] = (f"r32_{_n}_{_s}", _w())
    PICK[f"dp_count_f64_{_n}"] = (f"r64_{_n}_{_s}", _w(method="dp_count"))
    PICK[f"dp_value_f64_{_n}"] = (f"r64_{_n}_{_s}", _w(method="dp_value"))
for _n, _s in ((63, 4), (64, 5), (65, 6)):  # float32 rows through the dynamic program stay short: the reference's cumsum error grows with the row sum
    PICK[f"dp_count_f32_{_n}"] = (f"r32_{_n}_{_s}", _w(method="dp_count"))
    PICK[f"dp_value_f32_{_n}"] = (f"r32_{_n}_{_s}", _w(method="dp_value"))
PICK["greedy_f64_65"] = ("r64_65_6", _w())
PICK["greedy_f64_257"] = ("r64_257_9", _w())
for _m in METHODS:
    _t = "r32_257_9" if _m == "greedy" else "r64_257_9"
    PICK[f"own_max_{_m}"] = (_t, _w(pre_max=0, post_max=1, method=_m))  # every frame is its own maximum
    PICK[f"wide_row_{_m}"] = ("r32_65_6" if _m == "greedy" else "r64_65_6", _w(pre_max=100, post_max=200, pre_avg=300, post_avg=400, delta=0.1, method=_m))
    PICK[f"wide_tile_{_m}"] = ("r32_1292_10" if _m == "greedy" else "r64_1292_10", _w(pre_max=300, post_max=70, pre_avg=65, post_avg=400, delta=0.1, method=_m))
    PICK[f"plateau_{_m}"] = ("plateau300", _w(delta=0.25, wait=2, method=_m))
    PICK[f"frame0_{_m}"] = ("frame0_f32" if _m == "greedy" else "frame0_f64", _w(method=_m))
    PICK[f"delta0_{_m}"] = ("r32_257_9" if _m == "greedy" else "r64_257_9", _w(delta=0, method=_m))
    PICK[f"fraction_{_m}"] = ("r32_257_9" if _m == "greedy" else "r64_257_9", dict(pre_max=2.5, post_max=2.2, pre_avg=3.7, post_avg=4.1, delta=0.25, wait=3.5, method=_m))
for _wait in (0, 1, 63, 64, 65, 5000):  # the dead time within, at and across the 64-frame ballot chunks, and beyond the row
    PICK[f"wait{_wait}_greedy"] = ("r32_1292_10", _w(wait=_wait))
for _wait in (0, 63, 64, 65, 5000):
    PICK[f"wait{_wait}_dp_count"] = ("r64_1292_10", _w(wait=_wait, method="dp_count"))
    PICK[f"wait{_wait}_dp_value"] = ("r64_1292_10", _w(wait=_wait, method="dp_value"))
PICK["ring_dp_count"] = ("r64_4500_11", _w(wait=RING + 52, method="dp_count"))  # wait + 1 beyond the LDS ring: values from global scratch
PICK["ring_dp_value"] = ("r64_4500_11", _w(wait=RING + 52, method="dp_value"))
PICK["ring_edge_dp_value"] = ("r64_4500_11", _w(wait=RING - 1, method="dp_value"))  # wait + 1 == the ring
PICK["doc_plateau"] = ("doc_plateau", dict(pre_max=1, post_max=2, pre_avg=1, post_avg=2, delta=0, wait=0, sparse=False))
PICK["nan_greedy"] = ("nan257", _w())
PICK["batch_3x257"] = ("b32_3x257", _w(sparse=False))
PICK["batch_2x2x90_dp_value"] = ("b64_2x2x90", _w(sparse=False, method="dp_value"))
PICK["batch_2x2x90"] = ("b32_2x2x90", _w(sparse=False))
PICK["axis0"] = ("b32_257x3", _w(sparse=False, axis=0))

# exact by arithmetic (values on a dyadic grid: every sum is exact in either precision) or outside the mean's contract (NaN)
PICK_EXACT = tuple(f"plateau_{m}" for m in METHODS) + ("doc_plateau", "nan_greedy")

# ---- onset.onset_detect: name -> (input, kwargs).  "y:<key>": the signal; "env:<key>" / "env64:<key>": the reference's onset_strength of it
# (as float64), given as onset_envelope; "raw:<key>": an envelope used as it is.  energy "<key>": that input. -----------------------------
DETECT = {
    "y_mono": ("y:y0", dict()),
    "y_16k": ("y:y16", dict(_K16)),
    "y_f64": ("y:y0_f64", dict()),
    "y_batch4": ("y:pulses", dict(sparse=False)),
    "y_16k_samples": ("y:y16", dict(_K16, units="samples")),
    "y_16k_time": ("y:y16", dict(_K16, units="time")),
    "y_16k_frames": ("y:y16", dict(_K16, units="frames")),
    "y_backtrack": ("y:pulse96", dict(backtrack=True)),  # (y0's preceding minima do not survive the certification noise)
    "y_16k_backtrack": ("y:y16", dict(_K16, backtrack=True)),
    "env_f32": ("env:y0", dict()),
    "env_f64": ("env64:y0", dict()),
    "env_backtrack": ("env:y16", dict(_K16, backtrack=True)),
    "env_backtrack_energy": ("env:y16", dict(_K16, backtrack=True, energy="energy300")),  # a shorter energy: the late events lie past its end
    "env_raw_scale": ("env:y16", dict(_K16, normalize=False, delta=0.2)),
    "env_raw_backtrack": ("env:pulse96", dict(normalize=False, delta=1.0, backtrack=True)),
    "env_dp_count": ("env:y16", dict(_K16, method="dp_count")),
    "env_dp_value": ("env:y16", dict(_K16, method="dp_value")),
    "env_wait": ("env:y16", dict(_K16, wait=70, pre_max=8.5)),
    "env_batch4": ("env:pulses", dict(sparse=False)),
    "zero_sparse": ("raw:env_zero", dict()),
    "zero_time": ("raw:env_zero", dict(units="time")),
    "zero_dense": ("raw:env_zero2", dict(sparse=False)),
    "const_dense": ("raw:env_const2", dict(sparse=False)),  # constant rows normalise to zero
    "inf_row": ("raw:env_inf", dict()),
    "inf_dense": ("raw:env_inf2", dict(sparse=False)),
}

# ---- onset.onset_backtrack: name -> (events, energy key).  A case the reference refuses stores the exception's name instead. ------------
BACKTRACK = {
    "plain": ([3, 10, 17, 30, 49], "energy50"),
    "duplicates": ([10, 10, 11, 11, 12, 40, 40], "energy50"),
    "past_end": ([5, 49, 50, 60, 1000], "energy50"),
    "unsorted": ([40, 3, 22, 3], "energy50"),
    "negative": ([-1, 5, 10], "energy50"),
    "empty": ([], "energy50"),
    "len1": ([0, 1, 5], "energy1"),
    "len2": ([0, 1, 5], "energy2"),
    "len3": ([0, 1, 2, 5], "energy3"),
    "f64": ([3, 10, 17, 30, 49], "energy50_f64"),
    "flat": ([1, 4, 9, 15], "energy_flat"),  # equal neighbours: <= on the left, < on the right
}


def _row(n, seed, dtype):
    return np.abs(np.random.default_rng(9000 + seed).standard_normal(n)).astype(dtype)


def make_inputs():
    r = _rhythm_inputs()
    inp = dict(y0=r["y0"], y0_f64=r["y0_f64"], y16=r["y16"], pulses=r["pulses"], pulse96=r["pulses"][1])
    for key in sorted({k for k, _ in PICK.values()}):
        if key.startswith(("r32_", "r64_")):
            _, n, seed = key.split("_")
            inp[key] = _row(int(n), int(seed), np.float32 if key.startswith("r32") else np.float64)
    rng = np.random.default_rng(9100)
    inp["plateau300"] = (rng.integers(0, 8, size=300) / 4.0).astype(np.float32)
    inp["doc_plateau"] = np.array([0, 1, 1, 0, 2, 2, 2, 0, 1], np.float32)
    for dt, tag in ((np.float32, "f32"), (np.float64, "f64")):
        x = _row(130, 21, dt)
        x[0] = 5.0
        inp[f"frame0_{tag}"] = x
    x = _row(257, 22, np.float32)
    x[100] = np.nan
    inp["nan257"] = x
    inp["b32_3x257"] = _row(3 * 257, 23, np.float32).reshape(3, 257)
    inp["b32_2x2x90"] = _row(360, 24, np.float32).reshape(2, 2, 90)
    inp["b64_2x2x90"] = _row(360, 24, np.float64).reshape(2, 2, 90)
    inp["b32_257x3"] = _row(3 * 257, 25, np.float32).reshape(257, 3)
    inp["env_zero"] = np.zeros(100, np.float32)
    inp["env_zero2"] = np.zeros((2, 100), np.float32)
    inp["env_const2"] = np.full((2, 80), 1.5, np.float32)
    x = _row(120, 26, np.float32)
    x[50] = np.inf
    inp["env_inf"] = x
    inp["env_inf2"] = np.stack([_row(120, 27, np.float32), x])
    inp["energy300"] = _row(300, 28, np.float32)
    inp["energy50"] = _row(50, 29, np.float32)
    inp["energy50_f64"] = _row(50, 29, np.float64)
    inp["energy1"], inp["energy2"], inp["energy3"] = _row(1, 30, np.float32), np.array([2.0, 1.0], np.float32), np.array([2.0, 1.0, 3.0], np.float32)
    inp["energy_flat"] = np.array([3, 2, 2, 2, 3, 1, 1, 2, 2, 0, 0, 0, 5, 5, 4, 4, 6, 6], np.float32)
    return inp


def call_kwargs(kw, inputs):
    """The stored call description -> keyword arguments of a real call."""
    out = dict(kw)
    if isinstance(out.get("energy"), str):
        out["energy"] = inputs[out["energy"]]
    return out


def load():
    z = np.load(GOLDEN)
    inputs = make_inputs()
    for k, v in inputs.items():  # the seeds rebuild the reference's inputs exactly
        assert float(z[f"sum_{k}"]) == float(np.nansum(np.where(np.isfinite(v), v, 0.0), dtype=np.float64)), f"input {k} is not the one the fixture was made from"
    return z, json.loads(str(z["cases"])), inputs, json.loads(str(z["params"]))


def checksum(v):
    return np.float64(np.nansum(np.where(np.isfinite(v), v, 0.0), dtype=np.float64))


def detect_windows(sr, hop_length):
    """onset_detect's default picker arguments, after the ceilings: 30 ms / 0 ms, 100 ms / 100 ms, 30 ms, 0.07."""
    c = lambda v: int(np.ceil(v))  # noqa: E731
    return dict(pre_max=c(0.03 * sr // hop_length), post_max=c(0.00 * sr // hop_length + 1), pre_avg=c(0.10 * sr // hop_length), post_avg=c(0.10 * sr // hop_length + 1),
                wait=c(0.03 * sr // hop_length), delta=0.07)


def normalized(env):
    """onset_detect's normalisation, in the envelope's precision."""
    e = env - np.min(env, keepdims=True, axis=-1)
    e /= np.max(e, keepdims=True, axis=-1) + np.finfo(e.dtype).tiny
    return e


def window_facts(x, *, pre_max, post_max, pre_avg, post_avg):
    """Per frame of a one-dimensional row, in float64: is it the maximum of its window, the window's mean (summed first frame to last), the
    window's largest magnitude, its sum of magnitudes and its length."""
    x64 = np.asarray(x, dtype=np.float64)
    n = len(x64)
    idx = np.arange(n)
    mx = np.full(n, -np.inf)
    has_nan = np.zeros(n, bool)
    for k in range(-min(pre_max, n), min(post_max, n)):
        g = idx + k
        ok = (g >= 0) & (g < n)
        v = x64[np.clip(g, 0, n - 1)]
        has_nan |= ok & np.isnan(v)
        mx = np.where(ok & (v > mx), v, mx)
    is_max = (x64 == mx) & ~has_nan
    s = np.zeros(n)
    big = np.zeros(n)
    mag = np.zeros(n)
    cnt = np.zeros(n)
    for k in range(-min(pre_avg, n), min(post_avg, n)):
        g = idx + k
        ok = (g >= 0) & (g < n)
        v = np.where(ok, x64[np.clip(g, 0, n - 1)], 0.0)
        s = s + v
        big = np.maximum(big, np.where(np.isnan(v), 0.0, np.abs(v)))
        mag = mag + np.where(np.isnan(v), 0.0, np.abs(v))
        cnt += ok
    return is_max, s / cnt, big, mag, cnt


def greedy_model(x, *, pre_max, post_max, pre_avg, post_avg, delta, wait):
    """The greedy picker from its three conditions, in float64 on a one-dimensional row: x[n] is the maximum of x[n - pre_max : n + post_max],
    x[n] >= mean(x[n - pre_avg : n + post_avg]) + delta, and the previous peak lies more than ``wait`` frames back (earliest frames first).
    Window arguments are integers (after the ceiling).  Returns the bool row."""
    x64 = np.asarray(x, dtype=np.float64)
    is_max, mean, _, _, _ = window_facts(x64, pre_max=pre_max, post_max=post_max, pre_avg=pre_avg, post_avg=post_avg)
    with np.errstate(invalid="ignore"):
        cand = is_max & (x64 >= mean + delta)
    peaks = np.zeros(len(x64), bool)
    allowed = 0
    for i in np.flatnonzero(cand):
        if i >= allowed:
            peaks[i] = True
            allowed = i + wait + 1
    return peaks


def ceil_windows(kw):
    """The picker's integer arguments of a case's kwargs."""
    return dict(pre_max=int(np.ceil(kw["pre_max"])), post_max=int(np.ceil(kw["post_max"])), pre_avg=int(np.ceil(kw["pre_avg"])), post_avg=int(np.ceil(kw["post_avg"])),
                delta=float(kw["delta"]), wait=int(np.ceil(kw["wait"])))
