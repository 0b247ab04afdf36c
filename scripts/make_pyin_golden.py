"""Generate ``tests/golden/pyin.npz``: ``librosa.pyin`` and its observation stage (``__pyin_helper``) from the unmodified reference.

TEST INFRASTRUCTURE ONLY; runs only where the reference tree exists (through ``oracle/ref_shim``, imported read-only):

    python scripts/make_pyin_golden.py

Stored (``tests/pyin_cases.py`` has the cases and the rules):

* ``cmnd_tone`` / ``cmnd_noise``: the reference's float64 CMND of the two observation sources; per observation case the voiced half of
  ``__pyin_helper``'s ``observation_probs`` and its ``voiced_prob`` (the unvoiced half is ``(1 - voiced_prob) / P``, recomputed bit for bit);
* per end-to-end case the reference's ``f0``, ``voiced_flag`` and ``voiced_prob`` and, up to 242 states, the voiced half of its observation table;
* ``meta`` (JSON): digests of the inputs, each case's smallest distance from a rounding half, certification figures, refusal texts.

Certification of an end-to-end case: with ``delta`` the largest distance between the reference's CMND and the cancellation-free ``np.longdouble``
evaluation, every comparison of the observation stage on the model's CMND holds by more than ``CERT_FACTOR * delta``, every candidate's bin value
lies more than ``HALF_MARGIN + 1e4 * CERT_FACTOR * delta`` from a half (a shift moves by delta over the parabola's curvature, a bin by at most ten
per sample), and ``voiced_flag`` and the nan-filled ``f0`` are unchanged when the reference's log table is perturbed by 1e-12, eight seeds.
On failure the case's signal or seed is changed, not the bars.

As ``make_yin_golden.py`` does, this generator installs a per-element ``stencil`` after ``numba_standin.install()``.
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
import pyin_cases as PC  # noqa: E402
import yin_cases as YC  # noqa: E402


def main():
    librosa = ref_shim.load_reference()
    import librosa.core.pitch as ref_pitch
    import librosa.sequence as ref_sequence

    helper = getattr(ref_pitch, "__pyin_helper")

    def ref_front(y, kw):
        p0, p1 = YC.periods(kw)
        frames = np.array(YC.framed(y, **kw))
        cm = ref_pitch._cumulative_mean_normalized_difference(frames, p0, p1)
        return cm, ref_pitch._parabolic_interpolation(cm), frames, p0, p1

    def ref_obs(cm, sh, kw):
        p, nb, P = PC.obs_params(kw)
        thresholds, beta_probs = PC.prior(p["n_thresholds"], p["beta_parameters"])
        flat_c, flat_s = cm.reshape((-1,) + cm.shape[-2:]), sh.reshape((-1,) + sh.shape[-2:])
        with np.errstate(all="ignore"):
            out = [helper(c, s, p["sr"], thresholds, p["boltzmann_parameter"], beta_probs, p["no_trough_prob"], p["min_period"], p["fmin"], P, nb) for c, s in zip(flat_c, flat_s)]
        lead = cm.shape[:-2]
        return np.stack([o[0][0] for o in out]).reshape(lead + out[0][0].shape[1:]), np.stack([o[1][0] for o in out]).reshape(lead + out[0][1].shape[1:]), P

    out, meta = {}, {"obs": {}, "e2e": {}, "refusals": {}}

    # ---- (a) --------------------------------------------------------------------------------------------------------------------------------
    for src in PC.SOURCES:
        cm = ref_front(PC.source_signal(src), PC.OBS_KW)[0]
        assert cm.shape == (PC.N_LAGS, PC.SOURCES[src][1]) and cm.dtype == np.float64, cm.shape
        out["cmnd_" + src] = cm
    meta["synthetic"] = PC.digest(PC.synthetic_rows())
    events = set()
    for name in PC.OBS_CASES:
        kw = PC.obs_kw(name)
        cm, sh = PC.obs_inputs(name, out)
        p_ref, vp_ref, P = ref_obs(cm, sh, kw)
        p_mod, vp_mod, info = PC.obs_model(cm, sh, kw)
        assert np.allclose(p_mod, p_ref, rtol=1e-13, atol=0) and np.array_equal(p_mod == 0, p_ref == 0), (name, "the model differs from the reference")
        assert np.allclose(vp_mod, vp_ref, rtol=0, atol=1e-13), name
        assert info["half"] > PC.HALF_MARGIN, (name, info["half"], "a candidate is not settled: change the seed")
        assert np.array_equal(p_ref[..., P:, :], np.broadcast_to(((1 - vp_ref) / P)[..., None, :], p_ref[..., P:, :].shape)), name
        if PC.OBS_CASES[name]["src"] == "syn":
            events |= info["events"]
        out["obs_" + name], out["vp_" + name] = p_ref[..., :P, :], vp_ref
        meta["obs"][name] = dict(cmnd=PC.digest(cm), shifts=PC.digest(sh), half=info["half"], events=sorted(info["events"]), P=P, candidates=int((p_ref[..., :P, :] != 0).sum()))
        print(f"obs {name:16s} P {P:4d} candidates {meta['obs'][name]['candidates']:5d} half {info['half']:.2e} events {sorted(info['events'])}")
    assert events >= PC.SYN_EVENTS, PC.SYN_EVENTS - events

    # ---- (c) --------------------------------------------------------------------------------------------------------------------------------
    for name, c in PC.E2E_CASES.items():
        y, kw = PC.e2e_signal(name), c["kw"]
        y64 = y.astype(np.float64)
        hop = kw.get("hop_length") or kw.get("frame_length", 2048) // 4
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            f0, flag, vp = librosa.pyin(y64, **kw)
        cm, sh, frames, p0, p1 = ref_front(y64, kw)
        p_ref, vp_ref, P = ref_obs(cm, sh, kw)
        assert np.array_equal(vp_ref, vp), name
        # certification
        delta = float(np.max(np.abs(cm - YC.exact_cmnd(frames, p0, p1).astype(np.float64)), initial=0))
        cm_model = YC.model_cmnd(frames, p0, p1)
        margin, half = PC.comparison_margin(cm_model, YC.parabolic_shifts(cm_model), kw)
        assert margin > PC.CERT_FACTOR * delta, (name, margin, delta, "a comparison is within the reference's own error: change the seed")
        assert half > PC.HALF_MARGIN + 1e4 * PC.CERT_FACTOR * delta, (name, half, delta, "a bin is within the reference's own error: change the seed")
        transition, p_init, nb, P2 = PC.transition_tables(ref_sequence, kw, hop)
        assert P2 == P
        log_ref = np.log(p_ref + PC.TINY)
        base = PC.model_decode(log_ref, transition, p_init, 1e-4)
        f0_m, flag_m = PC.lookup(base, kw, np.nan)
        assert np.array_equal(flag_m, flag) and np.array_equal(f0_m, f0, equal_nan=True), (name, "the Viterbi model differs from the reference")
        for seed in range(PC.N_PERTURB):
            rng = np.random.default_rng(1000 + seed)
            st = PC.model_decode(log_ref + 1e-12 * rng.uniform(-1, 1, log_ref.shape), transition, p_init, 1e-4)
            f0_p, flag_p = PC.lookup(st, kw, np.nan)
            assert np.array_equal(flag_p, flag) and np.array_equal(f0_p, f0, equal_nan=True), (name, seed, "the outputs move under a 1e-12 perturbation: change the seed")
        out["f0_" + name], out["flag_" + name], out["vp_" + name] = f0, flag, vp
        if 2 * P <= 242:
            out["eobs_" + name] = p_ref[..., :P, :]
        meta["e2e"][name] = dict(y=PC.digest(y), states=2 * P, frames=int(f0.shape[-1]), voiced=int(flag.sum()), delta=delta, margin=margin, half=half)
        print(f"e2e {name:12s} states {2 * P:5d} frames {f0.shape[-1]:3d} voiced {int(flag.sum()):3d} delta {delta:.2e} margin {margin:.2e} half {half:.2e}")
    assert meta["e2e"]["e_zeros"]["voiced"] == 0 and not out["vp_e_zeros"].any()
    assert meta["e2e"]["e_one_frame"]["frames"] == 1 and meta["e2e"]["e_default"]["states"] == 1202
    assert 0 < meta["e2e"]["e_tone_gap"]["voiced"] < meta["e2e"]["e_tone_gap"]["frames"]

    # ---- (d) --------------------------------------------------------------------------------------------------------------------------------
    for name, (y, kw) in PC.refusal_calls().items():
        if name == "state_limit":   # (the reference accepts it; the device path's own limit)
            meta["refusals"][name] = None
            continue
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                librosa.pyin(y, **kw)
            meta["refusals"][name] = None
        except librosa.util.exceptions.ParameterError as exc:
            meta["refusals"][name] = str(exc)
        except Exception:  # noqa: BLE001  (fails incidentally in the reference: the package's own text is checked)
            meta["refusals"][name] = None
    print("refusals:", json.dumps(meta["refusals"], indent=1))

    out["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(PC.GOLDEN, **out)
    size = os.path.getsize(PC.GOLDEN)
    assert size < 1 << 20, size
    print("wrote", PC.GOLDEN, size, "bytes;", len(out) - 1, "arrays")


if __name__ == "__main__":
    main()
