"""Generate ``tests/golden/enhance.npz``: ``librosa.segment.path_enhance``, ``recurrence_to_lag``, ``lag_to_recurrence``, ``util.shear``,
``feature.stack_memory`` and ``filters.diagonal_filter`` from the unmodified reference.

TEST INFRASTRUCTURE ONLY; runs only where the reference tree exists (through ``oracle/ref_shim``, imported read-only), with SciPy:

    python scripts/make_enhance_golden.py

Inputs come from seeds (``tests/enhance_cases.py``).  Stored per case: the reference's result (``pe/``, ``lag/``, ``rec/``, ``shear/``,
``stack/``; bool as uint8), the ``diagonal_filter`` tables of a list of arguments (``filter/``), and in ``meta`` (JSON) the refusal texts and,
per ``path_enhance`` case, ``deviates``: whether the NumPy model differs from the reference in any bit, with the largest difference.

Certification: the model must equal the reference bit for bit on every lag, shear and stack case (they move values; there is nothing to round),
and is compared bit for bit on every ``path_enhance`` case; a case that differs is recorded, printed, and judged on the device by the bound of
a recursive sum instead (``enhance_cases.check_against_golden``).  The round trip ``lag_to_recurrence(recurrence_to_lag(x)) == x`` must hold
for the reference too.
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
sys.path.insert(0, ROOT)
import enhance_cases as EC  # noqa: E402

FILTER_ARGS = [("hann", 51, dict(slope=r)) for r in np.logspace(-1, 1, num=7, base=2)] + [
    ("hann", 1, {}), ("hann", 2, dict(slope=0.5)), ("hann", 4, dict(slope=2.0)), ("hann", 5, dict(slope=0.7)), ("hann", 8, dict(slope=1.5)), ("boxcar", 5, dict(slope=1.3)),
    ("hann", 7, dict(slope=1.0)), ("hann", 7, dict(angle=0.3)), ("hann", 9, dict(slope=0.6, zero_mean=True)), (("tukey", 0.5), 6, dict(slope=1.2)), ("hamming", 125, {})]


def stored(a):
    a = np.asarray(a)
    return a.astype(np.uint8) if a.dtype == np.bool_ else a


def main():
    ref = ref_shim.load_reference()
    import librosa.feature
    import librosa.filters
    import librosa.segment
    import librosa.util
    from librosa.util.exceptions import ParameterError

    out, meta = {}, {"pe": {}, "refusals": {}, "filters": []}
    t_all, failed = time.time(), []

    for i, (window, n, kw) in enumerate(FILTER_ARGS):
        out[f"filter/{i}"] = librosa.filters.diagonal_filter(window, n, **kw)
        meta["filters"].append(dict(window=window, n=n, kw={k: (float(v) if not isinstance(v, bool) else v) for k, v in kw.items()}))

    for name, c in EC.PE_CASES.items():
        R = EC.pe_input(name)
        before = R.copy()
        t0 = time.time()
        with np.errstate(all="ignore"):
            result = EC.pe_call(librosa.segment, name, R=EC.laid_out(R, c["layout"]))
        t_ref = time.time() - t0
        assert EC.same_bits(before, R) and result.dtype == R.dtype and result.shape == R.shape, name
        model = EC.pe_model(name)
        deviates = not EC.same_bits(model, result)
        diff = float(np.nanmax(np.abs(model.astype(np.float64) - result.astype(np.float64)), initial=0.0)) if deviates else 0.0
        out[f"pe/{name}"] = result
        meta["pe"][name] = dict(deviates=deviates, max_diff=diff)
        print(f"pe    {name:28s} {str(R.shape):16s} {R.dtype} reference {t_ref:6.2f} s  model {'DEVIATES by ' + str(diff) if deviates else 'equals the reference'}", flush=True)

    for name, c in EC.LAG_CASES.items():
        x = EC.lag_input(name)
        lag = librosa.segment.recurrence_to_lag(x.copy(), pad=c["pad"], axis=c["axis"])
        back = librosa.segment.lag_to_recurrence(lag, axis=c["axis"])
        assert EC.same_bits(back, x), f"{name}: the reference's round trip"
        if not EC.same_bits(EC.rec_to_lag_model(x, c["pad"], c["axis"]), lag) or not EC.same_bits(EC.lag_to_rec_model(lag, c["axis"]), back):
            failed.append(f"lag {name}: the model differs from the reference")
        out[f"lag/{name}"] = stored(lag)
    for name, c in EC.SHEAR_CASES.items():
        x = EC.shear_input(name)
        res = librosa.util.shear(x.copy(), factor=c["factor"], axis=c["axis"])
        if not EC.same_bits(EC.shear_model(x, c["factor"], c["axis"]), res):
            failed.append(f"shear {name}: the model differs from the reference")
        out[f"shear/{name}"] = stored(res)
    for name, c in EC.STACK_CASES.items():
        x = EC.stack_input(name)
        res = EC.stack_call(librosa.feature, name, data=x.copy())
        m = EC.stack_model(x, c["n_steps"], c["delay"], **c["kw"])
        if not EC.same_bits(m, res):
            failed.append(f"stack {name}: the model differs from the reference")
        out[f"stack/{name}"] = stored(res)
    print(f"{len(EC.LAG_CASES)} lag, {len(EC.SHEAR_CASES)} shear and {len(EC.STACK_CASES)} stack cases")

    for name, call in EC.refusals().items():
        try:
            call(ref)
        except ParameterError as e:
            meta["refusals"][name] = str(e)
        else:
            raise AssertionError(f"{name}: the reference accepted the call")
    assert not failed, "\n".join(failed)
    out["meta"] = np.array(json.dumps(meta))
    os.makedirs(os.path.dirname(EC.GOLDEN), exist_ok=True)
    np.savez_compressed(EC.GOLDEN, **out)
    n_dev = sum(e["deviates"] for e in meta["pe"].values())
    print(f"wrote {EC.GOLDEN}: {os.path.getsize(EC.GOLDEN)} bytes, {time.time() - t_all:.0f} s; the model equals the reference on {len(EC.PE_CASES) - n_dev} of {len(EC.PE_CASES)} "
          f"path_enhance cases")
    assert os.path.getsize(EC.GOLDEN) < 1024 * 1024


if __name__ == "__main__":
    main()
