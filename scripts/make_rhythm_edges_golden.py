"""Generate ``tests/golden/rhythm_edges.npz``: the reference's results at the edge cases of ``tests/rhythm_edges.py`` that the three older
rhythm fixtures do not reach (half-even tempi, frames per beat 1024 / 1025, win_length 2401, a ``max_size`` wider than 2 x bands, ...).

TEST INFRASTRUCTURE ONLY; runs only where the reference tree exists (through ``oracle/ref_shim``, imported read-only):

    python scripts/make_rhythm_edges_golden.py

It follows ``scripts/make_beat_golden.py``: ``scripts/numba_standin.py`` runs the tracker's numba kernels as the Python they are written in,
and every beat case is certified against the reference itself (8 noisy copies at radius 1e-5 give the same beats).  Inputs are rebuilt from
seeds by the tests; only their checksums and the results are stored.  Tempograms are stored as three sampled columns.  The reference cannot
track an all-zero row beside live rows, so the rows of a batch are run one by one and the all-zero row is stored without beats.
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
import rhythm_edges as E  # noqa: E402


def margins(score):
    """best - second best over axis -2; inf where at most one candidate is finite."""
    if score.shape[-2] < 2:
        return np.full(score.shape[:-2] + score.shape[-1:], np.inf)
    s = np.sort(np.where(np.isfinite(score), score, -np.inf), axis=-2)
    with np.errstate(invalid="ignore"):
        m = s[..., -1, :] - s[..., -2, :]
    return np.where(np.isnan(m), np.inf, m)


def track_row(librosa, env, bpm, case):
    """One row through the reference -> (dense beats, local score, cumulative score), certified."""
    call = dict(bpm=bpm, tightness=case["tightness"], trim=case["trim"], sparse=False, **E.BEAT_KW)
    numba_standin.LAST.clear()
    _, beats = librosa.beat.beat_track(onset_envelope=env, **call)
    ls = numba_standin.LAST["__beat_local_score"][0].copy()
    _, cum = numba_standin.LAST["__beat_track_dp"]
    cum = cum.copy()
    peak = float(np.max(np.abs(env)))
    for s in range(E.DRAWS):
        rng = np.random.default_rng(5000 + s)
        noisy = np.clip(env.astype(np.float64) + E.RADIUS * peak * rng.standard_normal(env.shape), 0.0, None).astype(env.dtype)
        assert np.array_equal(librosa.beat.beat_track(onset_envelope=noisy, **call)[1], beats), f"{case['name']}: not certified (replace the seed)"
    return np.asarray(beats), ls.reshape(env.shape), cum.reshape(env.shape)


def main():
    librosa = ref_shim.load_reference()
    import scipy

    x = np.array([1, 0, 1, 2, -1, 0, -2, 1])  # the stand-in's own check
    assert np.array_equal(librosa.util.localmax(x), [False, False, False, True, False, True, False, True])
    meta = dict(case="rhythm_edges", numpy=np.__version__, scipy=scipy.__version__, reference_version=str(librosa.__version__), radius=E.RADIUS, draws=E.DRAWS)
    store = {}

    for name in E.GOLDEN_TG:
        case = E.TG_CASES[name]
        env = E.tg_envelope(case)
        store[f"sum_tg_{name}"] = np.float64(E.checksum(env))
        tg = librosa.feature.tempogram(onset_envelope=env, win_length=case["W"], center=case["center"], norm=E.NORMS[case["norm"]])
        cols = E.golden_cols(tg.shape[-1])
        store[f"cols_tg_{name}"], store[f"tg_{name}"] = cols, tg[..., cols]
        if E.SUM in case["modes"]:
            kw = E.tempo_kwargs(case)
            bpms = librosa.tempo_frequencies(case["W"], hop_length=kw["hop_length"], sr=kw["sr"])
            with np.errstate(all="ignore"):
                lp = -0.5 * (np.log2(bpms) - np.log2(120.0)) ** 2
            lp[: int(np.argmax(bpms < 320.0))] = -np.inf
            for key, agg in (("mean", np.mean), ("none", None)):
                store[f"tempo_{key}_{name}"] = librosa.feature.tempo(onset_envelope=env, aggregate=agg, **kw)
                g = tg if agg is None else agg(tg, axis=-1, keepdims=True)
                with np.errstate(all="ignore"):
                    store[f"margin_{key}_{name}"] = margins(np.log1p(1e6 * g) + lp[:, None])
        print(f"tg    {name:22s} {tg.shape}", flush=True)

    for name in E.GOLDEN_BEAT:
        case = E.BEAT_CASES[name]
        env, bpm = E.beat_inputs(case)
        store[f"sum_beat_{name}"] = np.float64(E.checksum(env))
        if env.ndim == 1:
            beats, ls, cum = track_row(librosa, env, bpm, case)
        else:
            rows = [track_row(librosa, e, float(b), case) if e.any() else (np.zeros(e.shape, bool), np.zeros_like(e), np.full(e.shape, np.nan)) for e, b in zip(env, bpm)]
            beats, ls, cum = (np.stack([r[k] for r in rows]) for k in range(3))
        assert ls.dtype == env.dtype and cum.dtype == np.float64
        store[f"beats_beat_{name}"], store[f"ls_beat_{name}"], store[f"cum_beat_{name}"] = beats, ls, cum
        print(f"beat  {name:22s} {env.shape} {env.dtype}  {int(beats.sum())} beats", flush=True)

    for name in E.GOLDEN_ONSET:
        case = E.ONSET_CASES[name]
        S = E.onset_input(case)
        store[f"sum_onset_{name}"] = np.float64(E.checksum(S))
        store[f"onset_{name}"] = librosa.onset.onset_strength_multi(S=S, **E.onset_kwargs(case))
        print(f"onset {name:22s} {store[f'onset_{name}'].shape}", flush=True)

    np.savez_compressed(E.GOLDEN, params=json.dumps(meta), **store)
    print(E.GOLDEN, os.path.getsize(E.GOLDEN), "bytes")
    assert os.path.getsize(E.GOLDEN) < 1 << 20


if __name__ == "__main__":
    main()
