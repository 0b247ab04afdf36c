"""Generate ``tests/golden/beat.npz``: ``librosa.beat.beat_track`` outputs of the unmodified reference.

TEST INFRASTRUCTURE ONLY; runs only where the reference tree exists (through ``oracle/ref_shim``, imported read-only):

    python scripts/make_beat_golden.py [--no-full]

The reference's tracker is five numba kernels; ``scripts/numba_standin.py`` (installed before the shim's own stub) runs their undecorated
bodies.  This script asserts ``util.localmax``'s docstring example and the tracker's dtypes (local score float32, cumulative score float64,
back-links int32 for a float32 envelope), so a wrong stand-in cannot write fixtures silently.

Inputs come from seeds (``tests/beat_signals.py``; only checksums are stored).  Per case: the call (JSON), the reference's envelope
(``env_<case>``), tempo and beats, and for diagnosis ``ls_`` / ``cum_`` / ``bl_<case>`` (local score, cumulative score, back-links).

Certification: beats are a discrete decision, so equality can only be demanded where the decision is not balanced on a rounding error.
Every case is re-run on its envelope plus noise of ``RADIUS * max(envelope)`` (8 seeded draws, clipped at zero, cast back to the envelope's
dtype) and must give identical tempo and beats in all 8; the script asserts it.  ``RADIUS`` is stored in the file's params.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numba_standin  # noqa: E402

numba_standin.install()
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_shim  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import beat_signals as BS  # noqa: E402

RADIUS = 1e-5  # the onset change recorded a device-versus-reference envelope error of at most 3.1e-6 of the maximum in float32
DRAWS = 8
# A constant envelope has standard deviation 0, so after the normalisation any noise IS the signal: no radius certifies it and it has no
# seed to replace.  It stays in the fixture and in the equality tests (its input is exact there: a given envelope), flagged certified=false.
# Its stored values are not robust either (a local score near 1.4e38 in float32, every candidate of the recurrence tied after rounding).  If
# its equality test ever fails after a toolchain change while every certified case still passes, compare ls_ / cum_ of that case first: a
# one-ulp difference in exp is the expected cause, and then the case needs the issue's author, not a wider bound.
UNCERTIFIABLE = ("env_const",)


def same(a, b):
    (ta, ba), (tb, bb) = a, b
    return np.array_equal(np.asarray(ta), np.asarray(tb)) and np.array_equal(np.asarray(ba), np.asarray(bb))


def certify(librosa, env, call, want):
    peak = float(np.max(np.abs(env))) if env.size else 0.0
    for s in range(DRAWS):
        rng = np.random.default_rng(5000 + s)
        noisy = np.clip(env.astype(np.float64) + RADIUS * peak * rng.standard_normal(env.shape), 0.0, None).astype(env.dtype)
        if not same(librosa.beat.beat_track(onset_envelope=noisy, **call), want):
            return False
    return True


def main():
    librosa = ref_shim.load_reference()
    import scipy

    # the stand-in's own checks
    x = np.array([1, 0, 1, 2, -1, 0, -2, 1])
    assert np.array_equal(librosa.util.localmax(x), [False, False, False, True, False, True, False, True])
    x2 = np.array([[1, 0, 1], [2, -1, 0], [2, 1, 3]])
    assert np.array_equal(librosa.util.localmax(x2, axis=0), [[False, False, False], [True, False, False], [False, True, True]])

    meta = dict(numpy=np.__version__, scipy=scipy.__version__, reference_version=str(librosa.__version__), radius=RADIUS, draws=DRAWS)
    inputs = BS.make_inputs()
    store = {f"sum_{k}": np.float64(np.sum(v, dtype=np.float64)) for k, v in inputs.items()}
    cases = {}
    for name, (src, kw) in BS.CASES.items():
        kind, key = src.split(":")
        sr, hop = kw.get("sr", BS.SR), kw.get("hop_length", 512)
        if kind == "raw":
            env = inputs[key]
        else:
            env = librosa.onset.onset_strength(y=inputs[key], sr=sr, hop_length=hop, aggregate=np.median)
            if kind == "env64":
                env = env.astype(np.float64)
        if kw.get("bpm") == "frames":
            store[f"bpm_{name}"] = librosa.feature.tempo(onset_envelope=env, sr=sr, hop_length=hop, aggregate=None)
        call = BS.call_kwargs(kw, store, name)
        numba_standin.LAST.clear()
        want = librosa.beat.beat_track(onset_envelope=env, **call)
        if kind == "y":
            assert same(librosa.beat.beat_track(y=inputs[key], **call), want), name
        store[f"env_{name}"] = env
        store[f"tempo_{name}"] = np.asarray(want[0])
        store[f"beats_{name}"] = np.asarray(want[1])
        if "__beat_track_dp" in numba_standin.LAST:
            ls = numba_standin.LAST["__beat_local_score"][0]
            bl, cum = numba_standin.LAST["__beat_track_dp"]
            if env.dtype == np.float32:
                assert (ls.dtype, bl.dtype, cum.dtype) == (np.float32, np.int32, np.float64), (name, ls.dtype, bl.dtype, cum.dtype)
            store[f"ls_{name}"], store[f"cum_{name}"], store[f"bl_{name}"] = ls.copy(), cum.copy(), bl.copy()
        ok = certify(librosa, env, call, want)
        assert ok or name in UNCERTIFIABLE, f"{name}: not certified at radius {RADIUS} (replace the seed)"
        cases[name] = dict(input=src, kwargs=kw, certified=bool(ok))
        print(f"{name:14s} env {str(env.shape):10s} {env.dtype}  tempo {np.round(np.ravel(want[0])[:4], 2)}  beats {np.asarray(want[1]).sum() if np.asarray(want[1]).dtype == bool else len(want[1])}",
              flush=True)

    # the six converters (core/convert.py) on fixed arguments
    fr = np.array([0, 1, 7, 100, 2583])
    tm = np.array([0.0, 0.1, 0.5, 1.0, 3.3, 59.99])
    sm = np.array([0, 1, 511, 512, 513, 22050, 661500])
    store["conv_frames"], store["conv_times"], store["conv_samples"] = fr, tm, sm
    for hop, n_fft, sr in ((512, None, 22050), (160, 400, 16000), (441, 2048, 22050)):
        tag = f"{hop}_{n_fft}_{sr}"
        store[f"frames_to_samples_{tag}"] = librosa.frames_to_samples(fr, hop_length=hop, n_fft=n_fft)
        store[f"samples_to_frames_{tag}"] = librosa.samples_to_frames(sm, hop_length=hop, n_fft=n_fft)
        store[f"frames_to_time_{tag}"] = librosa.frames_to_time(fr, sr=sr, hop_length=hop, n_fft=n_fft)
        store[f"time_to_frames_{tag}"] = librosa.time_to_frames(tm, sr=sr, hop_length=hop, n_fft=n_fft)
        store[f"samples_to_time_{tag}"] = librosa.samples_to_time(sm, sr=sr)
        store[f"time_to_samples_{tag}"] = librosa.time_to_samples(tm, sr=sr)

    def save(full):
        out = BS.GOLDEN
        np.savez_compressed(out, params=json.dumps(dict(case="beat", full=full, **meta)), cases=json.dumps(cases), **store)
        print(out, os.path.getsize(out), "bytes", flush=True)

    save(False)
    if "--no-full" in sys.argv:
        return
    # the full-size batch: every row must have beats, and a median inter-beat interval within one frame of frames_per_beat for the returned tempo
    for i in range(BS.FULL_ROWS):
        env = librosa.onset.onset_strength(y=BS.full_signal(i), sr=BS.SR, hop_length=512, aggregate=np.median)
        want = librosa.beat.beat_track(onset_envelope=env, sr=BS.SR, hop_length=512)
        tempo, beats = want
        fpb = np.round(BS.SR / 512 * 60.0 / float(np.ravel(tempo)[0]))
        assert len(beats) >= 2 and abs(np.median(np.diff(beats)) - fpb) <= 1, (i, tempo, beats)
        if i in BS.FULL_STORED:
            assert certify(librosa, env, dict(sr=BS.SR, hop_length=512), want), f"full row {i}: not certified"
            store[f"full_env_{i}"], store[f"full_tempo_{i}"], store[f"full_beats_{i}"] = env, np.asarray(tempo), np.asarray(beats)
        print(f"full {i:3d}: {BS.full_bpm(i):6.1f} BPM -> tempo {float(np.ravel(tempo)[0]):6.1f}, {len(beats)} beats", flush=True)
    save(True)


if __name__ == "__main__":
    main()
