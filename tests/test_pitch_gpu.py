"""piptrack, pitch_tuning and estimate_tuning on the MI355X against tests/golden/pitch.npz (the unmodified reference) and the NumPy model of
tests/pitch_cases.py, under that module's bounds: the peak positions of ``piptrack(S=...)`` equal the reference's exactly and the values lie
within 4 ulp of the result dtype; on the certified signals the histogram's counts equal the float64 model's and ``estimate_tuning`` returns
the reference's float bit for bit.

Shapes are the smallest at which the kernels can go wrong (tests/pitch_cases.py): 2, 3, 33, 65, 257, 1025 and 2049 bins (2049 crosses the
1088-bin staging tile; the seam cases put a peak on each seam bin), 1, 63, 64, 65 and 300 frames, both layouts, three lead shapes, both
precisions, complex and signed input, every ref mode.

Measured on the MI355X (printed per case by the first test): the peak positions equal the reference's in every case and the worst value
error is 2 ulp (bound 4) in the two complex cases -- there the magnitude kernel's |z| stands in for ``np.abs`` -- and 0 or 1 ulp elsewhere; every counts row of the certified signals equals the float64 model's."""
import warnings

import numpy as np
import pytest

import librosa_amd as L
import pitch_cases as PC
from librosa_amd.core import pitch as pitch_mod

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    import json

    z = np.load(PC.GOLDEN)
    return z, json.loads(bytes(z["meta"]).decode())


def _torch():
    import torch

    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_like(A, pad=0):
    """A device tensor with the layout of ``A``: a frame-major view stays one (with ``pad`` unused elements behind every row)."""
    At = np.swapaxes(A, -1, -2)
    if A.ndim >= 2 and At.flags["C_CONTIGUOUS"] and not A.flags["C_CONTIGUOUS"]:
        if pad:
            buf = _torch().full(At.shape[:-1] + (At.shape[-1] + pad,), float("nan"), dtype=_dev(At[..., :1]).dtype, device="cuda")
            buf[..., : At.shape[-1]] = _dev(At)
            return buf[..., : At.shape[-1]].transpose(-1, -2)
        return _dev(At).transpose(-1, -2)
    return _dev(A)


def _quiet(fn):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn()


@pytest.mark.parametrize("name", list(PC.PIP))
def test_piptrack_of_a_spectrogram(golden, name):
    z, meta = golden
    S, kw = PC.pip_input(name), PC.pip_kwargs(name)
    assert PC.digest(S) == meta["inputs"][name]
    before = S.copy()
    got = L.piptrack(S=S, **kw)
    worst = 0.0
    for g, key in zip(got, ("pitches_", "mags_")):
        want = z[key + name]
        assert isinstance(g, np.ndarray) and g.shape == want.shape and g.dtype == want.dtype
        assert np.array_equal(g != 0, want != 0), (name, key, "peak positions")
        worst = max(worst, PC.ulp_distance(g, want))
    print(f"{name}: {worst:.3g} ulp, {int((got[0] != 0).sum())} peaks")
    assert worst <= PC.ULPS
    assert np.array_equal(S, before)
    pads = (0, 5) if PC.PIP[name]["layout"] == "fm" and PC.PIP[name]["kind"] != "complex" else (0,)
    for pad in pads:
        T = _dev_like(S, pad)
        t_before = T.clone()
        got_t = L.piptrack(S=T, **kw)
        for g, gt in zip(got, got_t):
            assert gt.is_cuda and tuple(gt.shape) == g.shape and np.array_equal(gt.cpu().numpy(), g)
        assert _torch().equal(T, t_before)
        if PC.PIP[name]["layout"] == "fm" and S.shape[-1] > 1 and S.shape[-2] > 1:
            assert got_t[0].stride(-2) == 1  # the view convention of stft / _spectrogram: frames major behind a (..., f, t) view


@pytest.mark.parametrize("name", ["r05_b12", "r05_b12_2ch"])
def test_piptrack_of_a_signal_is_piptrack_of_our_own_spectrogram(name):
    """``piptrack(y=...)`` against ``piptrack(S=...)`` of the magnitude spectrogram our own transform returns (``_spectrogram``, power 1)."""
    y = PC.tuning_signal(name)
    for arg in (y, _dev(y)):
        S, _ = L._spectrogram(y=arg, n_fft=PC.TUNE_N_FFT, hop_length=PC.TUNE_N_FFT // 4, power=1)
        a = L.piptrack(y=arg, sr=PC.SR, n_fft=PC.TUNE_N_FFT)
        b = L.piptrack(S=S, sr=PC.SR, n_fft=PC.TUNE_N_FFT)
        for u, v in zip(a, b):
            u, v = (u.cpu().numpy(), v.cpu().numpy()) if not isinstance(u, np.ndarray) else (u, v)
            assert u.shape == v.shape == y.shape[:-1] + (1025, 1 + y.shape[-1] // 512) and u.dtype == np.float32
            assert np.array_equal(u, v) and (u != 0).any()


@pytest.mark.parametrize("name", list(PC.TUNING))
def test_estimate_tuning_of_a_signal(golden, name):
    """The certification is re-run on our own spectrogram; then the counts are the float64 model's and the float is the reference's."""
    _, meta = golden
    y, kw = PC.tuning_signal(name), PC.tuning_kwargs(name)
    assert PC.digest(y) == meta["tuning"][name]["y"]
    S = np.ascontiguousarray(L._spectrogram(y=y, n_fft=kw["n_fft"], hop_length=kw["n_fft"] // 4, power=1)[0])
    skw = dict(sr=kw["sr"], n_fft=kw["n_fft"])
    assert PC.certify_tuning(S, kw["resolution"], kw["bins_per_octave"], **skw) == []
    want, counts = PC.model_estimate_tuning(S.astype(np.float64), kw["resolution"], kw["bins_per_octave"], **skw)
    assert want == meta["tuning"][name]["from_y"]
    for arg in (y, _dev(y)):
        row, _ = pitch_mod._tuning_row(arg, kw["sr"], None, kw["n_fft"], kw["resolution"], kw["bins_per_octave"], {})
        assert np.array_equal(row[:-2], counts) and row[-1] == meta["tuning"][name]["peaks"]
        got = L.estimate_tuning(y=arg, **kw)
        assert isinstance(got, float) and got == meta["tuning"][name]["from_y"]


@pytest.mark.parametrize("name", list(PC.TUNING))
def test_estimate_tuning_of_a_spectrogram(golden, name):
    _, meta = golden
    kw = PC.tuning_kwargs(name)
    S = PC.host_magnitudes(PC.tuning_signal(name))  # (certified by the host suite)
    assert PC.digest(S) == meta["tuning"][name]["S"]
    want, counts = PC.model_estimate_tuning(S.astype(np.float64), kw["resolution"], kw["bins_per_octave"], sr=kw["sr"], n_fft=kw["n_fft"])
    frame_major = np.swapaxes(np.ascontiguousarray(np.swapaxes(S, -1, -2)), -1, -2)
    rows = []
    for A in (S, frame_major, _dev_like(S), _dev_like(frame_major), _dev_like(frame_major, 7)):
        before = A.clone() if not isinstance(A, np.ndarray) else A.copy()
        row, _ = pitch_mod._tuning_row(None, kw["sr"], A, kw["n_fft"], kw["resolution"], kw["bins_per_octave"], {})
        rows.append(row)
        assert np.array_equal(row[:-2], counts) and row[-1] == meta["tuning"][name]["peaks"]
        again, _ = pitch_mod._tuning_row(None, kw["sr"], A, kw["n_fft"], kw["resolution"], kw["bins_per_octave"], {})
        assert np.array_equal(row, again), "two runs give the same counts"
        assert L.estimate_tuning(S=A, **kw) == meta["tuning"][name]["from_S"] == want
        assert np.array_equal(A, before) if isinstance(A, np.ndarray) else _torch().equal(A, before)
    assert all(np.array_equal(rows[0], r) for r in rows)


@pytest.mark.parametrize("name", list(PC.PIP))
def test_estimate_tuning_is_pitch_tuning_of_the_dense_result(name):
    """The fused route against the dense one selected on the host, bit for bit, counts included -- odd, even and zero peak counts occur."""
    S, kw = PC.pip_input(name), PC.pip_kwargs(name)
    for A in (S, _dev_like(S)):
        pitches, mags = L.piptrack(S=A, **kw)
        pitches, mags = (pitches.cpu().numpy(), mags.cpu().numpy()) if not isinstance(pitches, np.ndarray) else (pitches, mags)
        chosen, thr = PC.model_select(pitches, mags)
        for res, bpo in ((0.05, 12), (0.01, 36)):
            fused, _ = pitch_mod._tuning_row(None, kw["sr"], A, kw.get("n_fft", 2048), res, bpo, {k: v for k, v in kw.items() if k not in ("sr", "n_fft")})
            dense, _ = pitch_mod._pitch_tuning_row(chosen, res, bpo)
            assert fused[-1] == (pitches > 0).sum()
            if chosen.size == 0:
                assert dense is None and fused[-2] == 0 and not fused[:-2].any()
            else:
                assert np.array_equal(fused[:-1], dense[:-1]) and fused[-2] == chosen.size
            a = _quiet(lambda: L.estimate_tuning(S=A, resolution=res, bins_per_octave=bpo, **kw))
            b = _quiet(lambda: L.pitch_tuning(chosen, resolution=res, bins_per_octave=bpo))
            assert a == b


def test_silence_warns_and_returns_zero(golden):
    _, meta = golden
    assert meta["tuning"]["silence"] == dict(value=0.0, warned=["Trying to estimate tuning from empty frequency set."])
    for A in (np.zeros((1025, 6), np.float32), _dev(np.zeros((2, 65, 3), np.float64)), np.full((33, 4), 0.7, np.float32)):
        with pytest.warns(UserWarning, match="Trying to estimate tuning from empty frequency set."):
            assert L.estimate_tuning(S=A, sr=PC.SR) == 0.0
    with pytest.warns(UserWarning, match="Trying to estimate tuning from empty frequency set."):
        assert L.estimate_tuning(y=np.zeros(4096, np.float32), sr=PC.SR) == 0.0


@pytest.mark.parametrize("name", list(PC.PITCH_TUNING))
def test_pitch_tuning(golden, name):
    _, meta = golden
    c = PC.PITCH_TUNING[name]
    f, want = c["freqs"], meta["pitch_tuning"][name]
    for arg in (f, f.tolist(), _dev(f)) if f.size else (f,):
        if want["warned"]:
            with pytest.warns(UserWarning, match="Trying to estimate tuning from empty frequency set."):
                got = L.pitch_tuning(arg, **c["kw"])
        else:
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                got = L.pitch_tuning(arg, **c["kw"])
        assert isinstance(got, float) and got == want["value"], (name, got, want["value"])
    if f.size and (PC.pitch_tuning_margin(name) > (1e-4 if f.dtype == np.float32 else 1e-9) or name.startswith("fold")):
        row, _ = pitch_mod._pitch_tuning_row(f, c["kw"].get("resolution", 0.01), c["kw"].get("bins_per_octave", 12))
        assert np.array_equal(row[:-2], PC.model_pitch_tuning(f, **c["kw"])[1]) and row[-2] == (f > 0).sum()


def test_chroma_with_the_estimated_tuning_stays_on_the_device():
    y = _dev(PC.tuning_signal("r05_b12"))
    tuning = L.estimate_tuning(y=y, sr=PC.SR)
    assert isinstance(tuning, float) and -0.5 <= tuning < 0.5
    chroma = L.feature.chroma_stft(y=y, sr=PC.SR, tuning=tuning)
    assert chroma.is_cuda and tuple(chroma.shape) == (12, 1 + y.shape[-1] // 512) and bool(_torch().isfinite(chroma).all())
    assert np.array_equal(chroma.cpu().numpy(), L.feature.chroma_stft(y=y.cpu().numpy(), sr=PC.SR, tuning=tuning))
