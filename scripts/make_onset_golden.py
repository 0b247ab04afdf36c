"""Generate ``tests/golden/onset.npz``: ``librosa.onset.onset_strength`` / ``onset_strength_multi`` outputs of the reference.

TEST INFRASTRUCTURE ONLY; runs only where the reference tree exists (it goes through ``oracle/ref_shim``, which it imports read-only):

    python scripts/make_onset_golden.py

The file stores one stereo test signal (the other inputs are cut or cast from it), the small spectrograms of the ``S=`` cases,
every case's call (JSON, ``cases``) and the reference's result under the case's name.  For each mel configuration the cases use,
it also stores the reference's mel power spectrogram (``mel_<cfg>``) and its ``power_to_db`` (``db_<cfg>``), and for the case with a
custom ``feature`` that feature's output (``feature_out_<case>``), so that the host simulator test can feed the flux kernel the
reference's own input.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import golden_cases  # noqa: E402
import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "onset.npz")
SR = 22050


def test_signal():
    """~2 s of stereo noise + tone with a burst every 0.25 s (the envelope then has onsets to find)."""
    n = 2 * SR
    y = golden_cases.make_signal("mix", n, 41, (2,), "float32")
    t = np.arange(n)
    bursts = 1.0 + 3.0 * ((t % (SR // 4)) < 600) + 1.5 * (((t + 2000) % (SR // 3)) < 400)
    return (y * bursts[None, :] * 0.25).astype(np.float32)


def p75(x, axis):
    """The custom aggregate of the "p75" case (the tests define the same function)."""
    return np.percentile(x, 75, axis=axis)


def make_inputs(y):
    rng = np.random.default_rng(7)
    S_ref = (rng.standard_normal((2, 24, 40)) * 6.0 - 30.0).astype(np.float32)  # a dB-like spectrogram given as S, with a user ref
    R_ref = (S_ref + rng.standard_normal(S_ref.shape).astype(np.float32) * 3.0).astype(np.float32)
    S_small = (rng.standard_normal((10, 6)) * 4.0).astype(np.float32)
    S_nan = (rng.standard_normal((9, 12)) * 4.0).astype(np.float32)
    S_nan[4, 5] = np.nan
    S_nan[7, 9] = np.nan
    return dict(y=y, y0=y[0], y0_f64=y[0].astype(np.float64), y16=y[0, : 2 * 16000], S_ref=S_ref, R_ref=R_ref, S_small=S_small, S_nan=S_nan)


# name -> (function, input key, call kwargs, aggregate name, mel configuration or None)
# aggregate names: mean (default) / sum / max / min / median / false / p75 (the function above); channels given as slices are stored as
# {"slices": [[start, stop], ...]}
MEL = {
    "default": dict(src="y", kw=dict(sr=SR)),
    "lag2": dict(src="y0", kw=dict(sr=SR, n_fft=1024, hop_length=256, n_mels=64)),
    "hop441": dict(src="y0", kw=dict(sr=SR, n_fft=2048, hop_length=441)),
    "mixed400": dict(src="y16", kw=dict(sr=16000, n_fft=400, hop_length=160, n_mels=40)),
    "f64": dict(src="y0_f64", kw=dict(sr=SR)),
}
CASES = {
    "default": ("strength", "y", dict(), "mean", "default"),
    "lag2_max3": ("strength", "y0", dict(lag=2, max_size=3, n_fft=1024, hop_length=256, n_mels=64), "mean", "lag2"),
    "hop441": ("strength", "y0", dict(n_fft=2048, hop_length=441), "mean", "hop441"),
    "mixed400": ("strength", "y16", dict(sr=16000, n_fft=400, hop_length=160, n_mels=40), "mean", "mixed400"),
    "median_channels": ("multi", "y", dict(channels=[0, 32, 64, 96, 128]), "median", "default"),
    "max_slices": ("multi", "y", dict(channels={"slices": [[0, 40], [20, 90], [64, 128], [100, 101]]}), "max", "default"),
    "agg_false": ("multi", "y", dict(), "false", "default"),
    "sum": ("strength", "y", dict(), "sum", "default"),
    "min": ("strength", "y", dict(), "min", "default"),
    "detrend": ("strength", "y", dict(detrend=True), "mean", "default"),
    "nocenter": ("strength", "y", dict(center=False), "mean", "default"),
    "f64": ("strength", "y0_f64", dict(), "mean", "f64"),
    "median_f64_max3": ("multi", "y0_f64", dict(channels=[0, 50, 128], max_size=3, detrend=True), "median", "f64"),
    "S_given_ref": ("multi", "S_ref", dict(ref="R_ref", lag=2, channels=[0, 7, 24]), "mean", None),
    "S_lag_ge_frames": ("strength", "S_small", dict(lag=6), "mean", None),
    "S_lag_ge_frames_nocenter": ("strength", "S_small", dict(lag=8, center=False), "mean", None),
    "S_channels_odd": ("multi", "S_small", dict(channels=[1, 3, 3, 9]), "mean", None),
    "S_nan_mean": ("multi", "S_nan", dict(channels=[0, 3, 6, 9]), "mean", None),
    "S_nan_median": ("multi", "S_nan", dict(channels=[0, 3, 6, 9]), "median", None),
    "S_nan_max": ("multi", "S_nan", dict(channels=[0, 3, 6, 9]), "max", None),
    "S_nan_false": ("multi", "S_nan", dict(), "false", None),
    "p75": ("strength", "y", dict(), "p75", "default"),
    "feature_amp_mel": ("strength", "y0", dict(feature="amp_mel48", n_fft=1024, hop_length=256), "mean", None),
}


def aggregate_of(name):
    return dict(mean=np.mean, sum=np.sum, max=np.max, min=np.min, median=np.median, false=False, p75=p75)[name]


def call_kwargs(kw, inputs, lib):
    """The stored call description -> the keyword arguments of a real call (shared with the tests through the JSON)."""
    out = dict(kw)
    ch = out.get("channels")
    if isinstance(ch, dict):
        out["channels"] = [slice(a, b) for a, b in ch["slices"]]
    if isinstance(out.get("ref"), str):
        out["ref"] = inputs[out["ref"]]
    if out.get("feature") == "amp_mel48":
        def amp_mel48(*, y, sr, n_fft, hop_length, **k):
            return lib.feature.melspectrogram(y=y, sr=sr, n_fft=n_fft, hop_length=hop_length, power=1.0, n_mels=48, **k)
        out["feature"] = amp_mel48
    return out


def main():
    librosa = ref_shim.load_reference()
    import scipy

    meta = dict(numpy=np.__version__, scipy=scipy.__version__, reference_version=str(librosa.__version__))
    y = test_signal()
    inputs = make_inputs(y)
    store = {k: v for k, v in inputs.items() if k in ("y", "S_ref", "R_ref", "S_small", "S_nan")}
    for cfg, m in MEL.items():
        kw = dict(m["kw"])
        kw.setdefault("fmax", 0.5 * kw["sr"])  # what onset_strength_multi adds for its default feature
        M = librosa.feature.melspectrogram(y=inputs[m["src"]], **kw)
        store[f"mel_{cfg}"] = M
        store[f"db_{cfg}"] = librosa.power_to_db(np.abs(M))
    cases = {}
    for name, (fn, src, kw, agg, mel) in CASES.items():
        call = call_kwargs(kw, inputs, librosa)
        f = librosa.onset.onset_strength if fn == "strength" else librosa.onset.onset_strength_multi
        if src.startswith("S_"):
            res = f(S=inputs[src], aggregate=aggregate_of(agg), **call)
        else:
            res = f(y=inputs[src], aggregate=aggregate_of(agg), **call)
        store[name] = res
        if "feature" in call:  # the feature's own output too, for the simulator test (the decibel step is the kernel's)
            store[f"feature_out_{name}"] = call["feature"](y=inputs[src], sr=call.get("sr", SR), n_fft=call["n_fft"], hop_length=call["hop_length"])
        cases[name] = dict(fn=fn, input=src, kwargs=kw, aggregate=agg, mel=mel)
        print(f"{name:28s} {str(res.shape):14s} {res.dtype}")
    np.savez_compressed(OUT, params=json.dumps(dict(case="onset", **meta)), cases=json.dumps(cases), mel_configs=json.dumps(MEL), **store)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
