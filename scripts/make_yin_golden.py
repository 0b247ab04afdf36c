"""Generate ``tests/golden/yin.npz``: ``librosa.yin`` and its cumulative mean normalised difference function from the unmodified reference.

TEST INFRASTRUCTURE ONLY; runs only where the reference tree exists (through ``oracle/ref_shim``, imported read-only):

    python scripts/make_yin_golden.py

Inputs come from seeds (``tests/yin_cases.py``).  Stored per case: the reference's ``f0`` as it returns it and
``_cumulative_mean_normalized_difference`` in the input's dtype; in ``meta`` (JSON): the dtypes the reference returned, warning texts, SHA-256
digests of the inputs, ``eps`` (4 times the largest difference between the reference's float32 and float64 CMND of the case's samples),
``ref_f0_err`` (the largest relative distance, on settled frames, between the reference's float64 ``f0`` and a ``np.longdouble`` evaluation
of the cancellation-free difference function), ``ref_cmnd_err`` (the same for the CMND, every frame, relative to max(1, |c|)), the counts of settled, unsettled and silent frames, and the exception names of the refused calls.

The parabolic stencil's ``if`` does not survive ``scripts/numba_standin.py``'s whole-array ``stencil``; as ``make_pitch_golden.py`` does, this
generator installs a per-element ``stencil`` after ``numba_standin.install()``.

Certification (``tests/yin_cases.py``): at most 10 % of a case's non-silent frames and 3 % over all cases may be unsettled; on settled frames
the reference's float32 and float64 runs and the model must choose the same lag.  On failure the case's signal or seed is changed, not the bars.
"""
from __future__ import annotations

import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numba_standin  # noqa: E402

numba = numba_standin.install()


class _At:
    """x[k] inside a stencil body: the element k places from the current one."""

    def __init__(self, x, i):
        self.x, self.i = x, i

    def __getitem__(self, k):
        return self.x[self.i + k]


def _stencil(fn):
    """One-dimensional kernels with offsets -1 .. 1, evaluated element by element; both ends are zero."""

    def apply(x):
        x = np.asarray(x)
        out = np.zeros(len(x), dtype=np.result_type(x.dtype, np.float32))
        for i in range(1, len(x) - 1):
            out[i] = fn(_At(x, i))
        return out

    apply.__name__ = fn.__name__
    return apply


numba.stencil = _stencil
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_shim  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import yin_cases as YC  # noqa: E402


def main():
    librosa = ref_shim.load_reference()
    import librosa.core.pitch as ref_pitch

    def ref_cmnd(y, kw):
        p0, p1 = YC.periods(kw)
        return ref_pitch._cumulative_mean_normalized_difference(np.array(YC.framed(y, **kw)), p0, p1)

    out, meta = {}, {"cases": {}, "errors": {}}
    total = unsettled_total = 0
    for name, c in YC.CASES.items():
        y, kw = YC.signal(name), c["kw"]
        thr = kw.get("trough_threshold", 0.1)
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            f0 = librosa.yin(y, **kw)
        cmnd = ref_cmnd(y, kw)
        # the float32 run's own error: the same float32 samples through the reference in both precisions
        y32 = y.astype(np.float32)
        cm32, cm64 = ref_cmnd(y32, kw), ref_cmnd(y32.astype(np.float64), kw)
        eps = YC.EPS_FACTOR * float(np.max(np.abs(cm32.astype(np.float64) - cm64)))
        # the float64 model of the case's own samples decides what is settled
        y64 = y.astype(np.float64)
        m64 = YC.model(y64, **kw)
        ok = YC.settled(m64["cmnd"], thr, eps) & ~m64["silent"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            f0_64 = librosa.yin(y64, **kw)
            f0_32 = librosa.yin(y32, **kw)
        exact = YC.model(y64, exact=True, **kw)
        own = YC.model(y, **kw)
        # certification
        live = int((~m64["silent"]).sum())
        bad = live - int(ok.sum())
        assert bad <= YC.MAX_UNSETTLED_CASE * live, (name, bad, live)
        assert np.array_equal(exact["index"][ok], m64["index"][ok]), (name, "the exact evaluation chooses another lag on a settled frame")
        assert np.array_equal(own["index"][ok], m64["index"][ok]), (name, "the model in the input's dtype chooses another lag on a settled frame")
        assert np.max(YC.rel_err(own["f0"], f0), initial=0) <= 1e-12, (name, "the model differs from the reference")
        assert np.max(YC.rel_err(m64["f0"], f0_64), initial=0) <= 1e-12, (name, "the float64 model differs from the reference")
        assert np.allclose(own["cmnd"], cmnd, rtol=1e-6, atol=1e-9), (name, "the model's CMND differs from the reference's")
        lag32 = np.rint(kw["sr"] / f0_32 - m64["min_period"]).astype(np.int64)  # the shift stays within one bin: the rounded period names the lag ...
        near = np.abs(lag32 - m64["index"]) <= 1                                  # ... up to one, which the f0 distance below settles
        assert near[ok].all(), (name, "the reference's float32 run chooses another lag on a settled frame")
        if m64["silent"].any():
            assert np.all(f0[m64["silent"]] == kw["sr"] / m64["min_period"]), (name, "silent frames")
        ref_f0_err = float(np.max(YC.rel_err(f0_64[ok], exact["f0"][ok]), initial=0))
        ref_cmnd_err = float(np.max(YC.cmnd_err(ref_cmnd(y64, kw), exact["cmnd"]), initial=0))
        total += live
        unsettled_total += bad
        out["f0_" + name] = f0
        out["cmnd_" + name] = cmnd.astype(y.dtype)
        meta["cases"][name] = dict(y=YC.digest(y), f0_dtype=str(f0.dtype), cmnd_dtype=str(cmnd.dtype), warned=[str(w.message) for w in seen], eps=eps, ref_f0_err=ref_f0_err, ref_cmnd_err=ref_cmnd_err,
                                   frames=int(m64["silent"].size), silent=int(m64["silent"].sum()), unsettled=bad,
                                   f32_f0_err=float(np.max(YC.rel_err(f0_32[ok], m64["f0"][ok]), initial=0)),
                                   lags=[int(m64["index"][ok].min(initial=10**6)), int(m64["index"][ok].max(initial=-1))], n_lags=int(m64["cmnd"].shape[-2]))
        print(f"{name:22s} frames {m64['silent'].size:4d} silent {int(m64['silent'].sum()):3d} unsettled {bad:2d} eps {eps:.2e} ref_f0_err {ref_f0_err:.2e} "
              f"cmnd {ref_cmnd_err:.2e} f32_f0_err {meta['cases'][name]['f32_f0_err']:.2e} lags {meta['cases'][name]['lags']}")
    assert unsettled_total <= YC.MAX_UNSETTLED_ALL * total, (unsettled_total, total)
    meta["unsettled"], meta["live_frames"] = unsettled_total, total
    # the crafted cases land where they are meant to
    assert meta["cases"]["first_lag"]["lags"] == [0, 0], meta["cases"]["first_lag"]
    last = meta["cases"]["last_lag"]
    assert last["lags"] == [last["n_lags"] - 1] * 2, last
    assert meta["cases"]["two_periods_warning"]["warned"], "the warning case must warn"

    for name in YC.ERRORS:
        y, kw = YC.error_call(name)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                librosa.yin(y, **kw)
            meta["errors"][name] = None
        except Exception as exc:  # noqa: BLE001
            meta["errors"][name] = {"type": type(exc).__name__, "message": str(exc)}
    assert all(meta["errors"].values()), meta["errors"]

    out["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(YC.GOLDEN, **out)
    print("wrote", YC.GOLDEN, os.path.getsize(YC.GOLDEN), "bytes;", len(out) - 1, "arrays; unsettled", unsettled_total, "of", total)
    print("errors:", json.dumps(meta["errors"], indent=1))


if __name__ == "__main__":
    main()
