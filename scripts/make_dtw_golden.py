"""Generate ``tests/golden/dtw.npz``: ``librosa.sequence.dtw`` and ``dtw_backtracking`` from the unmodified reference.

TEST INFRASTRUCTURE ONLY; runs only where the reference tree exists (through ``oracle/ref_shim``, imported read-only):

    python scripts/make_dtw_golden.py

numba's ``jit`` is an identity under ``scripts/numba_standin.py``, so the accumulation runs as plain Python: the cases are kept small.  Inputs
come from seeds (``tests/dtw_cases.py``).  Stored per case: ``wp``, ``D[-1, :]`` and ``D[:, -1]``; in ``meta`` (JSON): the shape of ``D``, the
SHA-256 of the bytes of ``D`` and of ``steps``, per X/Y case its margin and ``delta``, and the message of every refused call.

Certification: the model must reproduce the reference's ``D``, ``steps`` and ``wp`` bit for bit on every case (for an X/Y case on the
reference's own cost matrix), and every X/Y case must have ``margin >= 1e-6`` and ``margin >= 4 * delta`` on the reference's path.  On failure
the case's seed is changed, not the bars.
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
import dtw_cases as DC  # noqa: E402


def reference_cost(X, Y, metric, subseq):
    """The cost matrix as the reference forms it (:368-397)."""
    from scipy.spatial.distance import cdist

    X, Y = np.atleast_2d(X), np.atleast_2d(Y)
    X, Y = np.swapaxes(X, -1, 0), np.swapaxes(Y, -1, 0)
    X, Y = X.reshape((X.shape[0], -1), order="F"), Y.reshape((Y.shape[0], -1), order="F")
    C = cdist(X, Y, metric=metric)
    return C.T if subseq and X.shape[0] > Y.shape[0] else C


def main():
    ref_shim.load_reference()
    import librosa.sequence as ref

    out, meta = {}, {"cases": {}, "refusals": {}, "backtracks": {}}
    for name, c in DC.CASES.items():
        t0 = time.time()
        a = DC.inputs(name)
        kw = a["kw"]
        if c["kind"] == "C":
            before = a["C"].copy()
            D, wp, steps = ref.dtw(C=a["C"], return_steps=True, **kw)
            assert np.array_equal(before, a["C"])
            C = a["C"]
        else:
            D, wp, steps = ref.dtw(a["X"], a["Y"], return_steps=True, **kw)
            C = reference_cost(a["X"], a["Y"], kw.get("metric", "euclidean"), kw.get("subseq", False))
        D, wp, steps = np.asarray(D), np.asarray(wp), np.asarray(steps)
        assert D.dtype == np.float64 and steps.dtype == np.int32 and wp.dtype == np.int64, (name, D.dtype, steps.dtype, wp.dtype)
        mD, mwp, mS = DC.model_dtw(C, kw)
        flipped = c["kind"] == "XY" and kw.get("subseq") and c["N"] > c["M"]
        if flipped:
            mwp = np.fliplr(mwp)
        assert np.array_equal(mD, D, equal_nan=True) and np.array_equal(np.signbit(mD), np.signbit(D)), f"{name}: the model's D differs from the reference's"
        assert np.array_equal(mS, steps), f"{name}: the model's steps differ from the reference's"
        assert np.array_equal(mwp, wp), f"{name}: the model's wp differs from the reference's"
        entry = dict(shape=list(D.shape), sha_D=DC.sha(D), sha_steps=DC.sha(steps))
        line = ""
        if c["kind"] == "XY":
            d = float(DC.delta(name, D))
            own = np.fliplr(wp) if kw.get("subseq") and (flipped or D.shape[0] > D.shape[1]) else wp
            g = float(DC.margin(C, kw, D, own))
            assert g >= DC.MARGIN_FLOOR and g >= DC.MARGIN_FACTOR * d, f"{name}: margin {g:.3g} fails certification (delta {d:.3g}); change its seed"
            # the NumPy cost matrix of the tests stays inside the bound it is judged by
            err = float(np.max(np.abs(DC.np_cost(a["X"], a["Y"], kw.get("metric", "euclidean")) - (C.T if flipped else C))))
            K = int(np.prod(c["lead"], dtype=int)) * c["K"]
            R = float(max(np.abs(a["X"]).max(), np.abs(a["Y"]).max()))
            assert err <= DC.eps_c(kw.get("metric", "euclidean"), K, R), (name, err)
            entry.update(margin=g, delta=d)
            line = f" margin {g:.3g} delta {d:.3g} np_cost off by {err:.3g}"
        out[f"{name}/wp"], out[f"{name}/row"], out[f"{name}/col"] = wp, D[-1].copy(), D[:, -1].copy()
        meta["cases"][name] = entry
        print(f"{name:22s} D {D.shape} wp {wp.shape}{line}  {time.time() - t0:.1f} s", flush=True)
    for name, (case, kw) in DC.BACKTRACKS.items():
        a = DC.inputs(case)
        S = DC.model(a["C"], a["kw"])[1]
        wp = np.asarray(ref.dtw_backtracking(S, **kw))
        table = DC.DEFAULT_STEPS if "step_sizes_sigma" not in kw else np.concatenate((DC.DEFAULT_STEPS, np.asarray(kw["step_sizes_sigma"])))
        assert np.array_equal(wp, DC.model_backtrack(S, table, kw.get("subseq", False), kw.get("start"))), f"{name}: the model's wp differs from the reference's"
        assert wp.dtype == np.int64
        out[f"{name}/wp"] = wp
        meta["backtracks"][name] = dict(length=int(len(wp)))
        print(f"{name:22s} wp {wp.shape}", flush=True)
    for name, (fn, args, kw, _) in DC.refusals().items():
        try:
            getattr(ref, fn)(*args, **kw)
        except ref.ParameterError as e:
            meta["refusals"][name] = str(e)
        else:
            raise AssertionError(f"{name}: the reference accepted the call")
    out["meta"] = np.array(json.dumps(meta))
    os.makedirs(os.path.dirname(DC.GOLDEN), exist_ok=True)
    np.savez_compressed(DC.GOLDEN, **out)
    print(f"wrote {DC.GOLDEN}: {os.path.getsize(DC.GOLDEN)} bytes, {len(DC.CASES)} cases")


if __name__ == "__main__":
    main()
