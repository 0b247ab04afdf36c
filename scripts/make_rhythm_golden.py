"""Generate ``tests/golden/rhythm.npz``: ``librosa.feature.tempogram`` / ``tempo`` outputs of the reference.

TEST INFRASTRUCTURE ONLY; runs only where the reference tree exists (it goes through ``oracle/ref_shim``, which it imports read-only):

    python scripts/make_rhythm_golden.py

Inputs are float32 signals and envelopes made from seeds (``tests/rhythm_signals.py``; only their checksums are stored).  Every case stores its call (JSON, ``cases``), the reference's onset
envelope (``env_<case>``, so the tests can feed the kernel exactly the reference's input) and its result.  Tempograms of the signal
cases are stored as a fixed sample of columns (``cols_<case>``, the padded edge frames included); tempo cases store the score margin
(best minus second best, per frame for ``aggregate=None``) in ``margin_<case>``.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ref_shim  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
from rhythm_signals import SR, call_kwargs, make_inputs  # noqa: E402  (the inputs are rebuilt from seeds by the tests too)

OUT = os.path.join(ROOT, "tests", "golden", "rhythm.npz")


# name -> (function, input key, kwargs).  Input keys starting with "y"/"silent"/"pulses" are signals (the reference computes the envelope);
# "env:<key>" uses the reference's onset envelope of that signal as onset_envelope; other keys are envelopes given as they are.
# window "ones" = np.ones; "win_array" = the stored array.  norm "inf" = np.inf.  aggregate "median" = np.median, "none" = None.
CASES = {
    "tg_y_stereo": ("tempogram", "y", dict(sr=SR)),
    "tg_y_f64": ("tempogram", "y0_f64", dict(sr=SR)),
    "tg_env_1d": ("tempogram", "env:y0", dict()),
    "tg_env_3d": ("tempogram", "env_rand", dict(win_length=64)),
    "tg_w344": ("tempogram", "env:y0", dict(win_length=344)),
    "tg_w127": ("tempogram", "env:y0", dict(win_length=127)),
    "tg_w8": ("tempogram", "env:y0", dict(win_length=8)),
    "tg_nocenter": ("tempogram", "env:y0", dict(win_length=127, center=False)),
    "tg_norm_none": ("tempogram", "env:y0", dict(win_length=127, norm=None)),
    "tg_norm_1": ("tempogram", "env:y0", dict(win_length=127, norm=1)),
    "tg_norm_2": ("tempogram", "env:y0", dict(win_length=127, norm=2)),
    "tg_norm_3": ("tempogram", "env:y0", dict(win_length=127, norm=3)),
    "tg_win_ones": ("tempogram", "env:y0", dict(win_length=127, window="ones")),
    "tg_win_array": ("tempogram", "env:y0", dict(win_length=127, window="win_array")),
    "tg_zero": ("tempogram", "env_zero", dict(win_length=32)),
    "tg_short": ("tempogram", "env_short", dict()),
    "tg_hop441": ("tempogram", "y0", dict(sr=SR, hop_length=441)),
    "tg_16k": ("tempogram", "y16", dict(sr=16000, hop_length=160)),
    "tempo_y": ("tempo", "y", dict(sr=SR)),
    "tempo_env": ("tempo", "env:y", dict(sr=SR)),
    "tempo_params": ("tempo", "y0", dict(sr=SR, start_bpm=90, std_bpm=0.5, max_tempo=None)),
    "tempo_prior": ("tempo", "y0", dict(sr=SR, prior="uniform")),
    "tempo_none": ("tempo", "y0", dict(sr=SR, aggregate="none")),
    "tempo_median": ("tempo", "y0", dict(sr=SR, aggregate="median")),
    "tempo_tg": ("tempo", "tg:y0", dict(sr=SR)),
    "tempo_silent": ("tempo", "silent", dict(sr=SR)),
    "tempo_pulses": ("tempo", "pulses", dict(sr=SR)),
    "tempo_16k": ("tempo", "y16", dict(sr=16000, hop_length=160)),
}
SAMPLE_COLS = 24  # stored tempogram columns of a signal case: the first and last 6 (the ramps) and 12 spread over the middle


def sample_cols(n):
    mid = np.linspace(6, n - 7, 12).round().astype(int) if n > 12 else np.arange(0)
    return np.unique(np.concatenate([np.arange(min(6, n)), mid, np.arange(max(n - 6, 0), n)])).astype(np.int64)


def margins(score):
    """best - second best over axis -2 (per remaining index); inf when one candidate alone is finite."""
    s = np.sort(np.where(np.isfinite(score), score, -np.inf), axis=-2)
    return s[..., -1, :] - s[..., -2, :]


def main():
    librosa = ref_shim.load_reference()
    import scipy

    meta = dict(numpy=np.__version__, scipy=scipy.__version__, reference_version=str(librosa.__version__))
    inputs = make_inputs()
    store = {f"sum_{k}": np.float64(np.sum(v, dtype=np.float64)) for k, v in inputs.items()}  # the tests check that they rebuild the same inputs
    cases = {}
    for name, (fn, src, kw) in CASES.items():
        call = call_kwargs(kw, inputs)
        sr, hop = call.get("sr", SR), call.get("hop_length", 512)
        sig = src.split(":")[-1]
        if src.startswith(("env:", "tg:")) or sig in ("y", "y0", "y0_f64", "y16", "silent", "pulses"):
            env = librosa.onset.onset_strength(y=inputs[sig], sr=sr, hop_length=hop)
        else:
            env = inputs[src]
        store[f"env_{name}"] = env
        if fn == "tempogram":
            if src.startswith("env:") or src in inputs and not src.startswith(("y", "silent", "pulses")):
                res = librosa.feature.tempogram(onset_envelope=env, **call)
            else:
                res = librosa.feature.tempogram(y=inputs[src], **call)
            if res.shape[-1] > 40:
                cols = sample_cols(res.shape[-1])
                store[f"cols_{name}"] = cols
                store[name] = res[..., cols]
            else:
                store[name] = res
        else:
            agg = call.pop("aggregate", np.mean)
            if src.startswith("tg:"):
                tg = librosa.feature.tempogram(onset_envelope=env, sr=sr, hop_length=hop)
                res = librosa.feature.tempo(tg=tg, aggregate=agg, **call)
            elif src.startswith("env:"):
                tg = librosa.feature.tempogram(onset_envelope=env, sr=sr, hop_length=hop, win_length=int(8.0 * sr) // hop)
                res = librosa.feature.tempo(onset_envelope=env, aggregate=agg, **call)
            else:
                tg = librosa.feature.tempogram(y=inputs[src], sr=sr, hop_length=hop, win_length=int(8.0 * sr) // hop)
                res = librosa.feature.tempo(y=inputs[src], aggregate=agg, **call)
            # the score the reference maximised, for the margin
            W = tg.shape[-2]
            bpms = librosa.tempo_frequencies(W, hop_length=hop, sr=sr)
            if call.get("prior") is None:
                lp = -0.5 * ((np.log2(bpms) - np.log2(call.get("start_bpm", 120))) / call.get("std_bpm", 1.0)) ** 2
            else:
                lp = call["prior"].logpdf(bpms)
            if call.get("max_tempo", 320.0) is not None:
                lp[: int(np.argmax(bpms < call.get("max_tempo", 320.0)))] = -np.inf
            g = tg if agg is None else agg(tg, axis=-1, keepdims=True)
            m = margins(np.log1p(1e6 * g) + lp[:, None])
            store[f"margin_{name}"] = m
            store[f"bpms_{name}"] = bpms
            store[f"logprior_{name}"] = lp
            if not src.startswith(("env", "tg")) and src != "silent":
                # aggregated: every estimate clear of the float32 envelope's tolerance; per frame (aggregate=None) the tests compare the frames
                # whose margin is, which must be most of them
                ok = np.mean(m >= 1e-3)
                assert (ok == 1.0) if agg is not None else (ok >= 0.9), f"{name}: score margins below 1e-3 ({1 - ok:.1%})"
            store[name] = res
        cases[name] = dict(fn=fn, input=src, kwargs=kw)
        print(f"{name:16s} {str(res.shape):16s} {res.dtype}  {'' if fn == 'tempogram' else np.round(res.ravel()[:6], 3)}")
    for W, hop, sr in ((384, 512, SR), (344, 512, SR), (800, 160, 16000), (8, 441, SR)):
        store[f"tempo_frequencies_{W}_{hop}_{sr}"] = librosa.tempo_frequencies(W, hop_length=hop, sr=sr)
        store[f"fourier_tempo_frequencies_{W}_{hop}_{sr}"] = librosa.fourier_tempo_frequencies(sr=sr, win_length=W, hop_length=hop)
    np.savez_compressed(OUT, params=json.dumps(dict(case="rhythm", **meta)), cases=json.dumps(cases), **store)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
