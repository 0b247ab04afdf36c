"""Generate ``tests/golden/chroma.npz``: ``librosa.filters.chroma`` / ``cq_to_chroma`` and ``librosa.feature.chroma_stft`` / ``chroma_cqt``
outputs of the unmodified reference.

TEST INFRASTRUCTURE ONLY; runs only where the reference tree exists (through ``oracle/ref_shim``, imported read-only):

    python scripts/make_chroma_golden.py

Inputs come from seeds (``tests/chroma_cases.py``); stored are the reference's results (``out_<group>_<case>``), the exception's name where
the reference refuses a call, and SHA-256 digests of the inputs and of every filter bank (``meta``, JSON) -- a digest pins a bank bit for bit
at 64 bytes instead of up to 200 KB.

``chroma_cqt(y=...)``: the reference's default converter needs ``soxr``; stored is ``chroma_cqt(C=|cqt(y, res_type="polyphase")|)`` of the
reference, which is what its ``y=`` form computes with that converter.

Certification.  Every stored result is asserted to lie within a tenth of the tests' bound (``chroma_cases.worst`` against the float64 model:
1e-4 / 1e-11 of the frame's largest element) -- for the ``y=`` cases the model starts from the float64 oracle transform of the signal.  For
every case with ``threshold > 0`` no float64 raw value may lie within ``1e-3 * threshold`` of the threshold.  On failure the seed is replaced
(``tests/chroma_cases.py``), not the bound.
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
import cqt_oracle as CQ  # noqa: E402
import stft_oracle as O  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import chroma_cases as CC  # noqa: E402

WORST = {}


def certify(name, ref, bank, x64, norm, threshold):
    out_dtype = ref.dtype
    mod, raw = CC.model(bank, x64, norm, threshold, out_dtype)
    w = CC.worst(ref, mod, out_dtype)
    WORST[name] = w
    assert w <= CC.bar(out_dtype) / 10, (name, w)
    if threshold is not None and threshold > 0:
        gap = np.abs(raw - threshold).min()
        assert gap > 1e-3 * threshold, (name, "raw value within 1e-3 of the threshold", gap)
        assert (raw < threshold).any() and (raw >= threshold).any(), (name, "the threshold decides nothing")


def main():
    librosa = ref_shim.load_reference()
    out, meta = {}, {"banks": {}, "cq_banks": {}, "inputs": {}, "errors": {}, "dtypes": {}}

    for name, kw in CC.BANKS.items():
        meta["banks"][name] = CC.digest(librosa.filters.chroma(**CC.bank_kwargs(kw)))
    for name, kw in CC.BANK_ERRORS.items():
        try:
            librosa.filters.chroma(**CC.bank_kwargs(kw))
            meta["errors"]["bank_" + name] = None
        except Exception as exc:  # noqa: BLE001
            meta["errors"]["bank_" + name] = type(exc).__name__
    for name, (n_input, kw) in CC.CQ_BANKS.items():
        try:
            meta["cq_banks"][name] = CC.digest(librosa.filters.cq_to_chroma(n_input, **CC.bank_kwargs(kw)))
        except Exception as exc:  # noqa: BLE001
            meta["cq_banks"][name] = type(exc).__name__
    # two small banks in full, so that a mismatch can be looked at
    out["bank_n64"] = librosa.filters.chroma(**CC.bank_kwargs(CC.BANKS["n64"]))
    out["cq_bank_b12_84"] = librosa.filters.cq_to_chroma(84)

    bank_keys = ("n_chroma", "tuning", "ctroct", "octwidth", "base_c", "dtype")
    for name, c in CC.STFT_S.items():
        S = CC.stft_s_input(name)
        kw = CC.call_kwargs(c["kw"])
        ref = librosa.feature.chroma_stft(S=S, **kw)
        bank = librosa.filters.chroma(sr=kw["sr"], n_fft=c["n_fft"], **{k: v for k, v in kw.items() if k in bank_keys})
        certify("s_" + name, ref, bank, S.astype(np.float64), kw.get("norm", CC.INF), None)
        out["out_s_" + name], meta["inputs"]["s_" + name] = ref, CC.digest(S)
    for name, c in CC.STFT_Y.items():
        y = CC.stft_y_input(name)
        kw = CC.call_kwargs(c["kw"])
        ref = librosa.feature.chroma_stft(y=y, **kw)
        bank = librosa.filters.chroma(sr=kw["sr"], n_fft=kw["n_fft"], **{k: v for k, v in kw.items() if k in bank_keys})
        skw = {k: v for k, v in kw.items() if k in ("n_fft", "hop_length", "win_length", "window", "center", "pad_mode")}
        S64 = np.abs(O.stft(y.astype(np.float64), **skw)) ** 2
        certify("y_" + name, ref, bank, S64, kw.get("norm", CC.INF), None)
        out["out_" + name], meta["inputs"][name] = ref, CC.digest(y)
    for name, c in CC.CQT_C.items():
        C = CC.cqt_c_input(name)
        kw = CC.call_kwargs(c["kw"])
        ref = librosa.feature.chroma_cqt(C=C, **kw)
        bank = librosa.filters.cq_to_chroma(C.shape[-2], **{k: v for k, v in kw.items() if k in ("bins_per_octave", "n_chroma", "fmin", "window")} | ({} if "bins_per_octave" in kw else {"bins_per_octave": 36}))
        certify("c_" + name, ref, bank, C.astype(np.float64), kw.get("norm", CC.INF), kw.get("threshold", 0.0))
        out["out_c_" + name], meta["inputs"]["c_" + name] = ref, CC.digest(C)
    for name, c in CC.CQT_Y.items():
        y = CC.cqt_y_input(name)
        kw = CC.call_kwargs(c["kw"])
        n_bins, bpo = CC.cqt_dims(kw)
        ckw = dict(sr=kw["sr"], n_bins=n_bins, bins_per_octave=bpo, tuning=kw["tuning"], res_type=CC.CQT_RES_TYPE)
        C_ref = np.abs(librosa.cqt(y, **ckw))
        ref = librosa.feature.chroma_cqt(C=C_ref, **{k: v for k, v in kw.items() if k not in ("sr", "tuning")})
        bank = librosa.filters.cq_to_chroma(n_bins, bins_per_octave=bpo)
        C64 = np.abs(CQ.cqt(y.astype(np.float64), **ckw))
        certify(name, ref, bank, C64, kw.get("norm", CC.INF), kw.get("threshold", 0.0))
        out["out_" + name], meta["inputs"][name] = ref, CC.digest(y)

    y = np.zeros(4096, np.float32)
    C84 = np.ones((84, 4), np.float32)
    for name, (fn, kw) in CC.ERRORS.items():
        kw = {k: (y if v == "y" else C84 if v == "C84" else v) for k, v in kw.items()}
        try:
            getattr(librosa.feature, fn)(**kw)
            meta["errors"][name] = None
        except Exception as exc:  # noqa: BLE001
            meta["errors"][name] = type(exc).__name__
    # the reference raises "Input must be finite" for every norm, None included
    bad = CC.stft_s_input("n512_t64").copy()
    bad[3, 5] = np.nan
    for norm in (CC.INF, None):
        try:
            librosa.feature.chroma_stft(S=bad, sr=CC.SR, tuning=0.0, norm=norm)
            meta["errors"][f"nan_norm_{norm}"] = None
        except Exception as exc:  # noqa: BLE001
            meta["errors"][f"nan_norm_{norm}"] = type(exc).__name__ + ": " + str(exc)

    meta["worst"] = WORST
    for k, v in out.items():
        meta["dtypes"][k] = str(v.dtype)
    out["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(CC.GOLDEN, **out)
    print("wrote", CC.GOLDEN, os.path.getsize(CC.GOLDEN), "bytes;", len(out) - 1, "arrays")
    print("errors:", meta["errors"])
    print("reference against the model, the six worst cases (fraction of the frame's largest element):")
    for k, v in sorted(WORST.items(), key=lambda kv: -kv[1])[:6]:
        print("  ", k, v)


if __name__ == "__main__":
    main()
