"""Generate ``tests/golden/pitch.npz``: ``librosa.piptrack`` / ``pitch_tuning`` / ``estimate_tuning`` outputs of the unmodified reference.

TEST INFRASTRUCTURE ONLY; runs only where the reference tree exists (through ``oracle/ref_shim``, imported read-only):

    python scripts/make_pitch_golden.py

Inputs come from seeds (``tests/pitch_cases.py``); stored are the reference's results, the exception's name where it refuses a call, and
SHA-256 digests of the inputs (``meta``, JSON).  The dense ``piptrack`` results are mostly zeros and compress to a few bytes per peak.

``scripts/numba_standin.py``'s ``stencil`` evaluates a kernel body on whole shifted arrays, which the ``if`` in the reference's parabolic
stencil does not survive; this generator installs a per-element ``stencil`` of its own after ``numba_standin.install()``.

Certification.  Every dense result must equal the NumPy model of ``pitch_cases`` in the same dtype (pattern exactly, values within 1 ulp).
Every ``estimate_tuning`` case must pass ``pitch_cases.certify_tuning`` -- on the case's ``S`` and, for the ``y=`` form, on the reference's
own spectrogram: magnitudes at the median cut more than 16 ulp apart, no residual within 1e-4 of a histogram edge, the winner ahead by at
least 3 counts.  Odd and even peak counts must both occur.  On failure the case's seed or signal is changed (``tests/pitch_cases.py``), not
the bars.
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
import pitch_cases as PC  # noqa: E402


def name_of(fn):
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        try:
            value = fn()
            return {"value": None if value is None else float(value), "warned": [str(w.message) for w in seen]}
        except Exception as exc:  # noqa: BLE001
            return {"error": type(exc).__name__}


def main():
    librosa = ref_shim.load_reference()
    out, meta = {}, {"inputs": {}, "tuning": {}, "pitch_tuning": {}, "errors": {}, "worst_ulp": {}, "peaks": {}}

    for name in PC.PIP:
        S = PC.pip_input(name)
        kw = PC.pip_kwargs(name)
        with np.errstate(all="ignore"):
            pitches, mags = librosa.piptrack(S=S, **kw)
            mp, mm = PC.model_piptrack(S, **kw)
        assert pitches.dtype == np.dtype(PC.PIP[name]["dtype"]) and pitches.shape == S.shape, name
        assert np.array_equal(pitches != 0, mp != 0) and np.array_equal(mags != 0, mm != 0), (name, "the model's peaks differ")
        worst = max(PC.ulp_distance(mp, pitches), PC.ulp_distance(mm, mags))
        assert worst <= 1, (name, worst)
        meta["worst_ulp"][name] = worst
        meta["peaks"][name] = int((pitches != 0).sum())
        meta["inputs"][name] = PC.digest(S)
        out["pitches_" + name], out["mags_" + name] = pitches, mags
    for must_peak in ("seam_fm", "last_fm", "shapes_bm", "ends_fm", "complex_bm", "negative_fm", "refmean_fm", "thr0_fm", "bins2049_fm", "bins3_bm"):
        assert meta["peaks"][must_peak] > 0, must_peak
    seam = out["pitches_seam_fm"]
    assert seam[PC.STAGE_TILE - 1, 0] > 0 and seam[PC.STAGE_TILE, 0] == 0 and seam[PC.STAGE_TILE, 1] > 0 and seam[PC.STAGE_TILE + 1, 2] > 0, "a peak on each seam bin"
    assert out["pitches_shapes_bm"][2, 0] > 0 and out["pitches_shapes_bm"][3, 0] == 0 and out["pitches_shapes_bm"][1, 4] > 0, "plateau and bin 1"
    last = out["pitches_last_fm"]
    assert (last[-1, ::2] > 0).all() and np.array_equal(out["mags_last_fm"][-1, ::2], PC.pip_input("last_fm")[-1, ::2]), "at the last bin mags == S"
    ends = out["pitches_ends_fm"]
    assert not ends[:3].any() and not ends[15:].any() and ends[3].any() and ends[14].any(), "fmin inclusive, fmax exclusive"

    parities = set()
    for name in PC.TUNING:
        y = PC.tuning_signal(name)
        kw = PC.tuning_kwargs(name)
        S = PC.host_magnitudes(y)
        skw = dict(sr=kw["sr"], n_fft=kw["n_fft"])
        why = PC.certify_tuning(S, kw["resolution"], kw["bins_per_octave"], **skw)
        assert not why, (name, "S", why)
        S_ref = np.abs(librosa.stft(y, n_fft=kw["n_fft"]))
        why = PC.certify_tuning(S_ref, kw["resolution"], kw["bins_per_octave"], **skw)
        assert not why, (name, "y", why)
        from_s = float(librosa.estimate_tuning(S=S, **kw))
        from_y = float(librosa.estimate_tuning(y=y, **kw))
        model, counts = PC.model_estimate_tuning(S.astype(np.float64), kw["resolution"], kw["bins_per_octave"], **skw)
        assert model == from_s, (name, model, from_s)
        n_peaks = int((PC.model_piptrack(S, **skw)[0] > 0).sum())
        parities.add(n_peaks % 2)
        meta["tuning"][name] = {"from_S": from_s, "from_y": from_y, "y": PC.digest(y), "S": PC.digest(S), "peaks": n_peaks, "lead": int(np.sort(counts)[-1] - np.sort(counts)[-2])}
    assert parities == {0, 1}, "odd and even peak counts must both occur"
    meta["tuning"]["silence"] = name_of(lambda: librosa.estimate_tuning(S=np.zeros((1025, 6), np.float32), sr=PC.SR))

    for name, c in PC.PITCH_TUNING.items():
        got = name_of(lambda: librosa.pitch_tuning(c["freqs"], **c["kw"]))
        if c["freqs"].size and (c["freqs"] > 0).any():
            assert got["value"] == PC.model_pitch_tuning(c["freqs"], **c["kw"])[0], name
        meta["pitch_tuning"][name] = dict(got, freqs=PC.digest(c["freqs"]))
    assert meta["pitch_tuning"]["cqt_quarter"]["value"] == 0.25

    y = np.zeros(4096, np.float32)
    for name, fn in {
        "no_input": lambda: librosa.piptrack(sr=PC.SR),
        "n_fft_none": lambda: librosa.piptrack(y=y, sr=PC.SR, n_fft=None),
        "one_bin": lambda: librosa.piptrack(S=np.ones((1, 4), np.float32), sr=PC.SR),
        "tuning_no_input": lambda: librosa.estimate_tuning(sr=PC.SR),
        "tuning_bad_kwarg": lambda: librosa.estimate_tuning(y=y, sr=PC.SR, nonsense=1),
    }.items():
        meta["errors"][name] = name_of(fn).get("error")

    out["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(PC.GOLDEN, **out)
    print("wrote", PC.GOLDEN, os.path.getsize(PC.GOLDEN), "bytes;", len(out) - 1, "arrays")
    print("errors:", meta["errors"])
    print("tuning:", json.dumps(meta["tuning"], indent=1))
    print("pitch_tuning:", {k: (v.get("value"), v.get("warned")) for k, v in meta["pitch_tuning"].items()})


if __name__ == "__main__":
    main()
