"""Generate ``tests/golden/peaks.npz``: ``librosa.util.peak_pick``, ``librosa.onset.onset_detect`` and ``librosa.onset.onset_backtrack``
outputs of the unmodified reference.

TEST INFRASTRUCTURE ONLY; runs only where the reference tree exists (through ``oracle/ref_shim``, imported read-only):

    python scripts/make_peak_golden.py [--no-full]

The reference's picker is three numba kernels; ``scripts/numba_standin.py`` (installed before the shim's own stub) runs their undecorated
bodies.  This script asserts the stand-in on the facts it relies on (a plateau row through all three methods, dense and sparse, and the
batch loop), so a wrong stand-in cannot write fixtures silently.

Inputs come from seeds (``tests/peak_cases.py``; only checksums are stored).  Per case: the call (JSON) and the reference's result
(``peaks_<case>`` / ``onsets_<case>`` / ``back_<case>``; the exception's name where the reference refuses the call), and for the
``onset_detect`` cases that start from a signal the reference's envelope (``env_<case>``).

Certification.  Peaks are discrete decisions.  The window maximum, ``==`` against it and the dynamic program's sums are exact in the reference
and on the device; the window mean is not: the reference rounds it to the row's precision (``np.mean`` for greedy, a ``cumsum`` difference for
the dynamic program), the device computes it in float64.  So for every frame that passes the maximum test this script computes the float64
slack ``|x[n] - mean - delta|`` and asserts that it is at least four times a bound on the reference's own rounding: with ``u = 2^-24``
(float32) or ``2^-53`` (float64) and window length ``L``, ``(L + 2) u max|x|`` for greedy and ``2 u sum|x| / L + 2 u max|x|`` for the dynamic
program, the sum over the row up to the window's end.  On failure the seed is replaced (``tests/peak_cases.py``), not the bound.  Rows on a
dyadic grid (every sum exact) and the NaN row are exempt and flagged ``exact``.  Cases that start from a signal or from the reference's
envelope also carry the device's envelope error: as in ``make_beat_golden.py`` the result must be identical on the envelope plus noise of
``RADIUS * max(envelope)`` over 8 seeded draws, clipped at zero.
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
import peak_cases as PC  # noqa: E402

RADIUS = 1e-5  # the value of beat.npz: the onset change recorded a device-versus-reference envelope error of at most 3.1e-6 of the maximum
DRAWS = 8
SAFETY = 4.0
SMALLEST = {}  # case -> (smallest slack, its bound)


def slack_ok(name, x, kw, method):
    """Every row of ``x``: the smallest slack of a frame that passes the maximum test against SAFETY times the reference's rounding bound."""
    x = np.asarray(x)
    u = 2.0**-24 if x.dtype == np.float32 else 2.0**-53
    w = PC.ceil_windows(kw)
    delta = w.pop("delta")
    w.pop("wait")
    ok = True
    for row in x.reshape(-1, x.shape[-1]):
        is_max, mean, big, mag, cnt = PC.window_facts(row, **w)
        if method == "greedy":
            bound = (cnt + 2) * u * big
        else:
            hi = np.minimum(np.arange(len(row)) + w["post_avg"], len(row))
            total = np.cumsum(np.abs(np.nan_to_num(row.astype(np.float64))))[hi - 1]
            bound = 2 * u * total / cnt + 2 * u * np.maximum(big, np.abs(delta))
        slack = np.abs(row.astype(np.float64) - mean - delta)
        sel = is_max & np.isfinite(slack)
        if sel.any():
            i = np.flatnonzero(sel)[np.argmin(slack[sel] / np.maximum(bound[sel], 1e-300))]
            if name not in SMALLEST or slack[i] / bound[i] < SMALLEST[name][0] / SMALLEST[name][1]:
                SMALLEST[name] = (float(slack[i]), float(bound[i]))
            ok &= bool(slack[i] >= SAFETY * bound[i])
    return ok


def result_of(fn):
    """The call's result, or the name of the exception the reference raises."""
    try:
        return np.asarray(fn())
    except Exception as exc:  # noqa: BLE001
        return np.asarray(type(exc).__name__)


def noise_ok(librosa, env, call, want):
    peak = float(np.max(np.abs(env))) if env.size else 0.0
    for s in range(DRAWS):
        rng = np.random.default_rng(7000 + s)
        noisy = np.clip(env.astype(np.float64) + RADIUS * peak * rng.standard_normal(env.shape), 0.0, None).astype(env.dtype)
        if not np.array_equal(np.asarray(librosa.onset.onset_detect(onset_envelope=noisy, **call)), want):
            return False
    return True


def main():
    librosa = ref_shim.load_reference()
    import scipy

    # the stand-in's own checks: the plateau (tied frames are all candidates), dense against sparse, and the loop over leading axes
    pl = np.array([0, 1, 1, 0, 2, 2, 2, 0, 1], np.float32)
    kw = dict(pre_max=1, post_max=2, pre_avg=1, post_avg=2, delta=0, wait=0)
    for method in PC.METHODS:
        dense = librosa.util.peak_pick(pl, sparse=False, method=method, **kw)
        assert dense.dtype == bool and np.array_equal(dense, [0, 1, 1, 0, 1, 1, 1, 0, 1]), (method, dense)
        assert np.array_equal(librosa.util.peak_pick(pl, method=method, **kw), np.flatnonzero(dense))
        assert np.array_equal(librosa.util.peak_pick(np.stack([pl, pl[::-1]]), sparse=False, method=method, **kw)[0], dense)
    assert np.array_equal(librosa.util.peak_pick(pl, **dict(kw, wait=1)), [1, 4, 6, 8])

    meta = dict(numpy=np.__version__, scipy=scipy.__version__, reference_version=str(librosa.__version__), radius=RADIUS, draws=DRAWS, safety=SAFETY)
    inputs = PC.make_inputs()
    store = {f"sum_{k}": PC.checksum(v) for k, v in inputs.items()}
    cases = {}
    failed = []

    for name, (key, kw) in PC.PICK.items():
        x = inputs[key]
        want = librosa.util.peak_pick(x, **kw)
        store[f"peaks_{name}"] = want
        exact = name in PC.PICK_EXACT
        rows = np.moveaxis(x, kw.get("axis", -1), -1)
        if not exact and not slack_ok(name, rows, kw, kw.get("method", "greedy")):
            failed.append(name)
        cases[name] = dict(kind="pick", input=key, kwargs=kw, exact=exact)
        print(f"{name:26s} {str(x.shape):12s} {x.dtype}  peaks {int(np.sum(want)) if want.dtype == bool else len(want)}  slack/bound {SMALLEST.get(name)}", flush=True)

    for name, (src, kw) in PC.DETECT.items():
        kind, key = src.split(":")
        sr, hop = kw.get("sr", PC.SR), kw.get("hop_length", 512)
        call = PC.call_kwargs(kw, inputs)
        if kind == "raw":
            env = inputs[key]
        else:
            env = librosa.onset.onset_strength(y=inputs[key], sr=sr, hop_length=hop)
            if kind == "env64":
                env = env.astype(np.float64)
            store[f"env_{name}"] = env
        before = env.copy()
        want = np.asarray(librosa.onset.onset_detect(onset_envelope=env, **call))
        assert np.array_equal(before, env, equal_nan=True), name  # the caller's array is not modified
        if kind == "y":
            assert np.array_equal(np.asarray(librosa.onset.onset_detect(y=inputs[key], **call)), want), name
        store[f"onsets_{name}"] = want
        certified = False
        if kind != "raw":
            pick = dict(PC.detect_windows(sr, hop), **{k: v for k, v in kw.items() if k in ("pre_max", "post_max", "pre_avg", "post_avg", "wait", "delta")})
            rows = PC.normalized(env) if kw.get("normalize", True) else env
            if not slack_ok(name, rows, pick, kw.get("method", "greedy")):
                failed.append(name)
            certified = noise_ok(librosa, env, call, want)
            if not certified:
                failed.append(name + " (noise)")
        cases[name] = dict(kind="detect", input=src, kwargs=kw, certified=bool(certified))
        print(f"{name:26s} {str(env.shape):12s} {env.dtype}  onsets {int(np.sum(want)) if want.dtype == bool else np.round(want[:6], 3)}  slack/bound {SMALLEST.get(name)}", flush=True)

    for name, (events, key) in PC.BACKTRACK.items():
        ev = np.asarray(events, dtype=np.int64)
        got = result_of(lambda: librosa.onset.onset_backtrack(ev, inputs[key]))
        store[f"back_{name}"] = got
        cases[name] = dict(kind="backtrack", events=events, energy=key)
        print(f"{name:26s} events {events} -> {got}", flush=True)
    # the minima rule behind every backtrack case: the whole row of preceding minima of the reference, for the simulator and the device
    for key in sorted({k for _, k in PC.BACKTRACK.values()} | {"energy300"}):
        m = len(inputs[key])
        store[f"prev_{key}"] = np.asarray(librosa.onset.onset_backtrack(np.arange(m), inputs[key])).astype(np.int32)
    for name in ("y_backtrack", "y_16k_backtrack", "env_backtrack", "env_raw_backtrack"):
        env = store[f"env_{name}"]
        rows = PC.normalized(env) if PC.DETECT[name][1].get("normalize", True) else env
        store[f"prev_{name}"] = np.asarray(librosa.onset.onset_backtrack(np.arange(len(env)), rows)).astype(np.int32)

    assert not failed, f"slack below {SAFETY} x the rounding bound (replace the seeds in tests/peak_cases.py): {failed}"
    worst = min(SMALLEST.items(), key=lambda kv: kv[1][0] / kv[1][1])
    print(f"smallest slack over bound: {worst[0]} {worst[1][0]:.3g} / {worst[1][1]:.3g}", flush=True)
    meta["smallest_slack"] = dict(case=worst[0], slack=worst[1][0], bound=worst[1][1])

    def save(full):
        out = PC.GOLDEN
        np.savez_compressed(out, params=json.dumps(dict(case="peaks", full=full, **meta)), cases=json.dumps(cases), **store)
        print(out, os.path.getsize(out), "bytes", flush=True)

    save(False)
    if "--no-full" in sys.argv:
        return
    # the stored rows of the full-size batch (256 x 30 s click trains): the reference's envelope and onsets, certified like the cases
    pick = PC.detect_windows(PC.SR, 512)
    for i in PC.FULL_STORED:
        env = librosa.onset.onset_strength(y=PC.full_signal(i), sr=PC.SR, hop_length=512)
        want = np.asarray(librosa.onset.onset_detect(onset_envelope=env, sr=PC.SR, hop_length=512))
        assert len(want) >= 10, (i, want)
        assert slack_ok(f"full_{i}", PC.normalized(env), pick, "greedy"), f"full row {i}: slack {SMALLEST[f'full_{i}']}"
        assert noise_ok(librosa, env, dict(sr=PC.SR, hop_length=512), want), f"full row {i}: not certified"
        store[f"full_env_{i}"], store[f"full_onsets_{i}"] = env, want
        print(f"full {i:3d}: {len(want)} onsets  slack/bound {SMALLEST[f'full_{i}']}", flush=True)
    save(True)


if __name__ == "__main__":
    main()
