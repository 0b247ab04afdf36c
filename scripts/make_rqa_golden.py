"""Generate ``tests/golden/rqa.npz``: ``librosa.sequence.rqa`` from the unmodified reference.

TEST INFRASTRUCTURE ONLY; runs only where the reference tree exists (through ``oracle/ref_shim``, imported read-only):

    python scripts/make_rqa_golden.py

numba's ``jit`` is an identity under ``scripts/numba_standin.py``, so the recurrence runs as plain Python: the cases are kept small.  Inputs come
from seeds (``tests/rqa_cases.py``).  Stored per case: ``path``, ``score[-1, :]`` and ``score[:, -1]``; in ``meta`` (JSON): the shape, the
SHA-256 of the bytes of ``score``, whether the reference's walk left the matrix, the two refusal texts, and the name of a binary case whose
maximum is attained in cells of different strips or row blocks.  bool and integer cases run the reference on ``sim.astype(float64)``.

Certification: the model must reproduce the reference's ``score`` bit for bit on every case, its ``path`` as the reference reads the pointers on
every case, and with the walk along the scored moves on every case whose reference walk stays inside the matrix.  Only the two quirk cases may
leave it; any other case that does gets another seed.
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numba_standin  # noqa: E402

numba_standin.install()
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_shim  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import rqa_cases as RC  # noqa: E402


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(f"u{a.itemsize}"), b.view(f"u{b.itemsize}"))


def main():
    ref_shim.load_reference()
    import librosa.sequence as ref

    out, meta = {}, {"cases": {}, "refusals": {}, "tie_case": None}
    t_all = time.time()
    for name, c in RC.CASES.items():
        t0 = time.time()
        sim = RC.inputs(name)
        given = sim if sim.dtype.kind == "f" else sim.astype(np.float64)
        before = given.copy()
        with np.errstate(invalid="ignore", over="ignore"):
            score, path = ref.rqa(given, **RC.kwargs(name))
            only = ref.rqa(given, backtrack=False, **RC.kwargs(name))
        score, path = np.asarray(score), np.asarray(path)
        assert np.array_equal(before, given, equal_nan=True) and same_bits(np.asarray(only), score)
        assert score.dtype == RC.expected_dtype(name) and path.dtype == np.uint64 and path.ndim == 2 and path.shape[1] == 2, (name, score.dtype, path.dtype, path.shape)
        m_score, m_path, m_ptr = RC.model_rqa(sim, **RC.kwargs(name))
        assert same_bits(m_score, score), f"{name}: the model's score differs from the reference's"
        as_reference, left = RC.walk(m_score, m_ptr, reference=True)
        assert np.array_equal(as_reference, path), f"{name}: the model's reading of the reference's walk differs from the reference's path"
        assert left == (name in RC.QUIRKS), f"{name}: the reference's walk {'left' if left else 'stayed inside'} the matrix; change the seed"
        if not left:
            assert np.array_equal(m_path, path), f"{name}: the model's path differs from the reference's"
        if c["kind"] == "binary" and meta["tie_case"] is None:
            rows, strip = RC.geometry(name)
            at = np.argwhere(score == np.nanmax(score))
            if len({(int(i) // rows, int(j) // strip) for i, j in at}) >= 2:
                meta["tie_case"] = name
        out[f"{name}/path"], out[f"{name}/row"], out[f"{name}/col"] = path, score[-1].copy(), score[:, -1].copy()
        meta["cases"][name] = dict(shape=list(score.shape), sha_score=RC.sha(score), left=bool(left), length=int(len(path)))
        print(f"{name:48s} score {score.shape} path {path.shape}{' LEFT' if left else ''}  {time.time() - t0:.2f} s", flush=True)
    assert meta["tie_case"] is not None, "no binary case attains its maximum in two strips or row blocks"
    for name, kw in RC.refusals().items():
        try:
            ref.rqa(np.ones((4, 5)), **kw)
        except ref.ParameterError as e:
            meta["refusals"][name] = str(e)
        else:
            raise AssertionError(f"{name}: the reference accepted the call")
    out["meta"] = np.array(json.dumps(meta))
    os.makedirs(os.path.dirname(RC.GOLDEN), exist_ok=True)
    np.savez_compressed(RC.GOLDEN, **out)
    print(f"wrote {RC.GOLDEN}: {os.path.getsize(RC.GOLDEN)} bytes, {len(RC.CASES)} cases, tie case {meta['tie_case']}, {time.time() - t_all:.0f} s")


if __name__ == "__main__":
    main()
