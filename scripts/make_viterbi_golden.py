"""Generate ``tests/golden/viterbi.npz``: ``librosa.sequence``'s Viterbi decoders and transition builders from the unmodified reference.

TEST INFRASTRUCTURE ONLY; runs only where the reference tree exists (through ``oracle/ref_shim``, imported read-only):

    python scripts/make_viterbi_golden.py

numba's ``jit`` is an identity under ``scripts/numba_standin.py``, so ``_viterbi`` runs as plain Python: the cases are kept small.  Inputs come
from seeds (``tests/viterbi_cases.py``).  Stored per case: the reference's states and ``logp`` exactly as it returns them (``_viterbi`` itself,
sequence by sequence, for the log-domain cases); in ``meta`` (JSON): per case the margin of the decoded path and ``delta`` (the module
docstring of ``viterbi_cases``), the message of every refused call and of every refused builder call.  The builders' tables are stored as they
come.

Certification: every public-path case must have ``margin >= 1e-6`` and ``margin >= 4 * delta``, and the model must reproduce the reference's
states and ``logp`` bit for bit on every case.  On failure the case's seed is changed, not the bars.
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
import viterbi_cases as VC  # noqa: E402


def main():
    ref_shim.load_reference()
    import librosa.sequence as ref

    out, meta = {}, {"cases": {}, "refusals": {}, "builder_errors": {}}
    for name, c in VC.CASES.items():
        t0 = time.time()
        a = VC.inputs(name)
        if c["fn"] == "log":
            lead, S, T = c["lead"], c["S"], c["T"]
            lt = a["log_trans"] if a["log_trans"] is not None else VC.band_dense(S)
            res = [ref._viterbi(np.ascontiguousarray(x.T), lt, a["log_p_init"], a["thr"]) for x in a["log_prob"].reshape((-1, S, T))]
            states = np.stack([r[0] for r in res]).reshape(lead + (T,))
            logp = np.stack([r[1] for r in res]).reshape(lead + (1,))
        else:
            fn = {"viterbi": ref.viterbi, "discriminative": ref.viterbi_discriminative, "binary": ref.viterbi_binary}[c["fn"]]
            before = a["prob"].copy()
            states, logp = fn(a["prob"], a["transition"], return_logp=True, **a["kw"])
            assert np.array_equal(before, a["prob"])
        states, logp = np.asarray(states), np.asarray(logp)
        assert states.dtype == np.uint16 and logp.dtype == np.float64, (name, states.dtype, logp.dtype)
        assert (states.shape, logp.shape) == VC.out_shapes(name), (name, states.shape, logp.shape, VC.out_shapes(name))
        m_states, m_logp, margin = VC.model_case(name)
        assert np.array_equal(m_states.reshape(states.shape), states), f"{name}: the model's states differ from the reference's"
        assert np.array_equal(m_logp.reshape(logp.shape), logp, equal_nan=True), f"{name}: the model's logp differs from the reference's"
        d = VC.delta(name, logp)
        if c["fn"] != "log":
            assert margin >= VC.MARGIN_FLOOR and margin >= VC.MARGIN_FACTOR * d, f"{name}: margin {margin:.3g} fails certification (delta {d:.3g}); change its seed"
        out[f"{name}/states"], out[f"{name}/logp"] = states, logp
        meta["cases"][name] = dict(margin=float(margin) if np.isfinite(margin) else None, delta=float(d))
        print(f"{name:22s} states {states.shape} logp {logp.shape} margin {margin:.3g} delta {d:.3g}  {time.time() - t0:.1f} s", flush=True)
    for name, (fn, args, kw) in VC.BUILDERS.items():
        out[f"builder/{name}"] = getattr(ref, fn)(*args, **kw)
    for name, (fn, args, kw) in VC.BUILDER_ERRORS.items():
        try:
            getattr(ref, fn)(*args, **kw)
        except ref.ParameterError as e:
            meta["builder_errors"][name] = str(e)
        else:
            raise AssertionError(f"{name}: the reference accepted the call")
    for name, (fn, prob, transition, kw, _) in VC.refusals().items():
        try:
            getattr(ref, fn)(prob, transition, **kw)
        except ref.ParameterError as e:
            meta["refusals"][name] = str(e)
        else:
            raise AssertionError(f"{name}: the reference accepted the call")
    out["meta"] = np.array(json.dumps(meta))
    os.makedirs(os.path.dirname(VC.GOLDEN), exist_ok=True)
    np.savez_compressed(VC.GOLDEN, **out)
    print(f"wrote {VC.GOLDEN}: {os.path.getsize(VC.GOLDEN)} bytes, {len(VC.CASES)} cases")


if __name__ == "__main__":
    main()
