"""Generate ``tests/golden/knn.npz``: ``librosa.segment.recurrence_matrix`` and ``cross_similarity`` from the unmodified reference.

TEST INFRASTRUCTURE ONLY; runs only where the reference tree exists (through ``oracle/ref_shim``, imported read-only), with scikit-learn and SciPy:

    python scripts/make_knn_golden.py

Inputs come from seeds (``tests/knn_cases.py``).  Stored per case: the reference's dense result (bool as uint8) and, for a
``recurrence_matrix(mode="connectivity")`` whose ``k`` does not cover every candidate, the pattern of its ``mode="distance"`` result.  In ``meta``
(JSON), per case: ``ref_dev``, the reference's largest deviation of a stored distance from the ``longdouble`` model (relative; absolute for
``cosine``); ``aff_factor``, ``max(distance / bandwidth) + 1``, and ``inv_bw``, the largest ``1 / bandwidth`` of an
entry, both read off the reference's own affinities and distances; ``margin``, the smallest relative gap between the
last kept and the first dropped candidate distance; and the reference's refusal texts.

Certification: the model's pattern must equal the expected pattern on every case (``knn_cases.expected_pattern``), the margin must exceed 1000
times the value tolerance (else: another seed, recorded in ``knn_cases.RESEED``), the duplicate cases must hold exact zeros that the reference
dropped, and the counts of how often the reference's connectivity pattern differs from its own distance pattern are printed.
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_shim  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_cases as KC  # noqa: E402


def as_dense(r):
    if hasattr(r, "toarray"):
        assert type(r).__name__ == "csc_array" and r.indices.dtype == np.int32, (type(r), r.indices.dtype)
        r = r.toarray()
    return np.asarray(r)


def main():
    ref_shim.load_reference()
    import librosa.segment as ref
    from librosa.util.exceptions import ParameterError

    out, meta = {}, {"cases": {}, "refusals": {}}
    differ = {"rec": [0, 0], "cross": [0, 0]}
    t_all, failed = time.time(), []
    for name, c in KC.CASES.items():
        data, data_ref = KC.inputs(name)
        kw = KC.kwargs(name)
        mode = kw.get("mode", "connectivity")
        before = data.copy()
        try:
            result = as_dense(KC.call(ref, name))
        except ParameterError as e:
            meta["cases"][name] = dict(refused=str(e))
            print(f"{name:100s} refused: {e}")
            continue
        assert np.array_equal(before, data)
        assert result.dtype == (np.bool_ if mode == "connectivity" else np.float64), (name, result.dtype)
        Q = KC.frames(data, kw.get("axis", -1))
        R = Q if c["fn"] == "rec" else KC.frames(data_ref)
        n, n_ref = Q.shape[1], R.shape[1]
        k, _, width = KC.plan(c["fn"], n, n_ref, kw)
        cuts = k < (n_ref - width)
        # the reference's distances for the same arguments: its deviation from the exact model, and the pattern a cutting connectivity case is judged by
        kw_d = dict(kw, mode="distance", sparse=False)
        kw_d.pop("bandwidth", None)
        kw_d.pop("self", None)
        if mode == "connectivity":
            kw_d.pop("full", None)   # (no effect on connectivity; on distance it would replace k)
        dist = np.asarray(ref.recurrence_matrix(data, **kw_d) if c["fn"] == "rec" else ref.cross_similarity(data, data_ref, **kw_d))
        exact = KC.distances(Q, R, c["metric"], real=np.longdouble).T
        at = dist != 0
        if c["metric"] == "cosine":
            ref_dev = float(np.max(np.abs(dist[at] - exact[at]), initial=0.0))
        else:
            ref_dev = float(np.max(np.abs(dist[at] - exact[at]) / np.abs(exact[at]), initial=0.0))
        if mode == "connectivity":
            differ[c["fn"]][1] += 1
            differ[c["fn"]][0] += int(not np.array_equal(result & ~np.eye(*result.shape, dtype=bool), at & ~np.eye(*result.shape, dtype=bool)))
            if c["fn"] == "rec" and cuts:
                out[f"{name}/pattern"] = at.astype(np.uint8)
        out[f"{name}/result"] = result.astype(np.uint8) if result.dtype == np.bool_ else result
        stored = result[result > 0]   # (not the NaN that exp(0 / -0) leaves where the bandwidth is 0: those must be NaN on the device too)
        aff_factor = float(np.max(-np.log(stored), initial=0.0) + 1.0) if mode == "affinity" else 1.0
        both = (result > 0) & (dist > 0) if mode == "affinity" else np.zeros(result.shape, bool)
        inv_bw = float(np.max(-np.log(result[both]) / dist[both], initial=0.0))   # 1 / bandwidth of an entry, read off the reference's own affinity and distance
        skip_zero = c["fn"] == "rec" and mode != "connectivity"
        margin = KC.margins(exact.T, k, width, skip_zero)
        meta["cases"][name] = dict(ref_dev=ref_dev, aff_factor=aff_factor, inv_bw=inv_bw, margin=margin if np.isfinite(margin) else None, shape=list(result.shape), stored=int((result != 0).sum()))
        KC._loaded = (out, meta)
        rel, ab = KC.value_tolerance(name)
        if margin <= 1000 * max(rel, ab):
            failed.append(f"{name}: margin {margin:.3g} is within 1000 x {max(rel, ab):.3g}: change the seed")
        m_result, m_D = KC.model(name)
        want = KC.expected_pattern(name)
        if not np.array_equal(m_result != 0, want):
            failed.append(f"{name}: the model's pattern differs from the reference's in {int(((m_result != 0) != want).sum())} entries")
        if name in KC.DUPLICATES:
            assert (m_D == 0).sum() > n, f"{name}: no exact zero distances"
            dropped = (m_D.T == 0) & (result == 0) & ~np.eye(*result.shape, dtype=bool)
            assert dropped.any(), f"{name}: the reference did not return exact zeros for the duplicates"
        print(f"{name:100s} {str(result.shape):10s} stored {meta['cases'][name]['stored']:6d} ref_dev {ref_dev:.2e} margin {margin:.2e}", flush=True)
    for name in KC.refusals():
        try:
            KC.refusal_call(ref, name)
        except ParameterError as e:
            meta["refusals"][name] = str(e)
        else:
            raise AssertionError(f"{name}: the reference accepted the call")
    assert not failed, "\n".join(failed)
    meta["connectivity_differs_from_distance"] = differ
    out["meta"] = np.array(json.dumps(meta))
    os.makedirs(os.path.dirname(KC.GOLDEN), exist_ok=True)
    np.savez_compressed(KC.GOLDEN, **out)
    print(f"wrote {KC.GOLDEN}: {os.path.getsize(KC.GOLDEN)} bytes, {len(KC.CASES)} cases, {time.time() - t_all:.0f} s; connectivity pattern differs from the distance pattern in "
          f"{differ['rec'][0]} of {differ['rec'][1]} recurrence_matrix and {differ['cross'][0]} of {differ['cross'][1]} cross_similarity cases")


if __name__ == "__main__":
    main()
