"""chroma_stft and chroma_cqt on the MI355X against tests/golden/chroma.npz and the float64 model of tests/chroma_cases.py, under the
project's bound: |got - model| <= 1e-4 (float32) / 1e-11 (float64) of the largest element of the frame.

Shapes are the smallest at which the kernels can go wrong (tests/chroma_cases.py): bin counts off the wave width (33, 201, 257, 501, 1025,
2049), frame counts 1, 63, 64, 65, 70 (64 + 6: off the 4 frames a wave carries at once, kFr) and 130 (2 x 64 + 2: off the workgroup's tile of
64 frames, kTileF), 300 (more than one 256-frame workgroup of the bin-major form), n_chroma 5 / 12 / 36 / 50 (50: five chunks of kRows = 12
rows), both layouts of S / C, every norm, float64 input and a float64 bank.

Measured on the MI355X (maximum over the cases of each group, as a fraction of the frame's largest element; printed per case by the tests):
frame-major form 2.96e-7 (batch3_c50), bin-major form 2.84e-6 (2049 bins summed in order by one thread; 1.66e-6 at 1025 bins),
chroma_stft(y=...) 3.14e-7 (7.2e-7 at most against the reference's own result), chroma_cqt(y=...) 3.87e-7, float64 1.44e-15."""
import numpy as np
import pytest

import chroma_cases as CC
import librosa_amd as L
import stft_oracle as O
from librosa_amd import filters
from librosa_amd.core import spectrum
from librosa_amd.feature import chroma as chroma_mod

pytestmark = pytest.mark.gpu

chroma_stft, chroma_cqt = L.feature.chroma_stft, L.feature.chroma_cqt


@pytest.fixture(scope="module")
def golden():
    return CC.load()


def _torch():
    import torch

    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _frame_major(X):
    """The same values behind a view of a [..., t, f] array: what the library's own _spectrogram returns."""
    return np.swapaxes(np.ascontiguousarray(np.swapaxes(X, -1, -2)), -1, -2)


def _both_layouts(fn, X, name, mod, out_dtype):
    """``fn(array or tensor)`` on the C-contiguous array (bin-major kernel) and on the frame-major view (frame-major kernel), NumPy and device
    tensor each: under the bound, NumPy and tensor bit for bit the same, the input untouched.  Returns the two results."""
    res = []
    for form, A in (("bin-major", np.ascontiguousarray(X)), ("frame-major", _frame_major(X))):
        before = A.copy()
        got = fn(A)
        assert isinstance(got, np.ndarray) and got.dtype == out_dtype and got.shape == mod.shape
        w = CC.worst(got, mod, out_dtype)
        print(f"{name} {form}: {w:.3g} of the frame's maximum")
        assert w <= CC.bar(out_dtype), (name, form, w)
        T = _dev(A.swapaxes(-1, -2)).transpose(-1, -2) if form == "frame-major" else _dev(A)
        assert T.stride() == tuple(s // A.itemsize for s in A.strides) or A.size <= 1 or 1 in A.shape
        t_before = T.clone()
        got_t = fn(T)
        assert got_t.is_cuda and np.array_equal(got_t.cpu().numpy(), got)
        assert np.array_equal(A, before) and _torch().equal(T, t_before)
        res.append(got)
    return res


@pytest.mark.parametrize("name", list(CC.STFT_S))
def test_chroma_stft_of_a_spectrogram(golden, name):
    z, _ = golden
    c, S = CC.STFT_S[name], CC.stft_s_input(name)
    kw = CC.call_kwargs(c["kw"])
    bank = filters.chroma(**CC.stft_bank_kwargs(kw, c["n_fft"]))
    out_dtype = CC.result_dtype(S.dtype, bank.dtype)
    mod, _ = CC.model(bank, S, kw.get("norm", CC.INF), None, out_dtype)
    ref = z["out_s_" + name]
    assert ref.dtype == out_dtype and CC.worst(ref, mod, out_dtype) <= CC.bar(out_dtype) / 10
    res = _both_layouts(lambda A: chroma_stft(S=A, **kw), S, name, mod, out_dtype)
    if c.get("zero"):  # lengths below tiny: left as they are, exactly zero, no NaN
        for got in res:
            assert not np.any(got[1]) and not np.any(got[0][:, c["frames"] // 3 : c["frames"] // 3 + 9]) and np.isfinite(got).all()


@pytest.mark.parametrize("name", list(CC.STFT_Y))
def test_chroma_stft_of_a_signal(golden, name):
    """The power STFT (fused power-of-two: 64 / 512 / 2048 / 4096; mixed-radix: 400; rocFFT: 1000) chained into the chroma kernel."""
    z, _ = golden
    c, y = CC.STFT_Y[name], CC.stft_y_input(name)
    kw = CC.call_kwargs(c["kw"])
    skw = {k: v for k, v in kw.items() if k in ("n_fft", "hop_length", "win_length", "window", "center", "pad_mode")}
    S64 = np.abs(O.stft(y.astype(np.float64), **skw)) ** 2
    bank = filters.chroma(**CC.stft_bank_kwargs(kw, kw["n_fft"]))
    mod, _ = CC.model(bank, S64, kw.get("norm", CC.INF), None, np.float32)
    before = y.copy()
    got = chroma_stft(y=y, **kw)
    assert got.dtype == np.float32 and got.shape == z["out_" + name].shape
    w = CC.worst(got, mod, np.float32)
    print(f"{name}: {w:.3g} of the frame's maximum; against the reference's result {CC.worst(got, z['out_' + name].astype(np.float64), np.float32):.3g}")
    assert w <= CC.F32_BAR
    got_t = chroma_stft(y=_dev(y), **kw)
    assert got_t.is_cuda and np.array_equal(got_t.cpu().numpy(), got) and np.array_equal(y, before)
    if c["lead"]:
        for i in range(c["lead"][0]):  # a clip alone: the bits of the clip in the batch
            assert np.array_equal(chroma_stft(y=y[i], **kw), got[i])


def test_chroma_stft_float64_bank_over_float32_audio():
    y = CC.stft_y_input("y_n512")
    kw = dict(CC.call_kwargs(CC.STFT_Y["y_n512"]["kw"]), dtype=np.float64)
    got = chroma_stft(y=y, **kw)
    S = L._spectrogram(y=y, n_fft=512, hop_length=128, power=2)[0]
    mod, _ = CC.model(filters.chroma(sr=CC.SR, n_fft=512, dtype=np.float64), S, CC.INF, None, np.float64)
    assert got.dtype == np.float64 and CC.worst(got, mod, np.float64) <= CC.F64_BAR
    got_t = chroma_stft(y=_dev(y), **kw)
    assert got_t.dtype == _torch().float64 and np.array_equal(got_t.cpu().numpy(), got)


def test_chroma_stft_float64_audio():
    y = CC.stft_y_input("y_n400").astype(np.float64)
    kw = CC.call_kwargs(CC.STFT_Y["y_n400"]["kw"])
    got = chroma_stft(y=y, **kw)
    S64 = np.abs(O.stft(y, n_fft=400, hop_length=100)) ** 2
    mod, _ = CC.model(filters.chroma(sr=CC.SR, n_fft=400), S64, CC.INF, None, np.float64)
    w = CC.worst(got, mod, np.float64)
    print(f"float64 audio: {w:.3g}")
    assert got.dtype == np.float64 and w <= CC.F64_BAR


@pytest.mark.parametrize("n_fft,hop,n", [(2048, 512, 512 * 69), (4096, 1024, 1024 * 19)])
def test_chroma_stft_reads_the_padded_device_view_in_place(monkeypatch, n_fft, hop, n):
    """row_align=128: the rows of a device-resident spectrogram are padded to whole cache lines behind the (..., f, t) view."""
    torch = _torch()
    y = _dev(CC.signal(50, (2,), n))
    n_bins = 1 + n_fft // 2
    monkeypatch.setattr(spectrum, "ROW_ALIGN_BYTES", 128)
    S = L._spectrogram(y=y, n_fft=n_fft, hop_length=hop, power=2)[0]
    monkeypatch.undo()
    pitch = spectrum.row_pitch(n_bins, 4, 128)
    assert pitch > n_bins and S.stride(-2) == 1 and S.stride(-1) == pitch  # the padded view
    D = L.stft(y, n_fft=n_fft, hop_length=hop, row_align=128)
    assert D.stride(-1) == spectrum.row_pitch(n_bins, 8, 128) > n_bins
    S2 = D.abs() ** 2  # (whatever layout torch gives the result of the two element-wise operations)
    bank = filters.chroma(sr=CC.SR, n_fft=n_fft)
    for name, view in (("padded power view", S), ("stft(row_align=128).abs() ** 2", S2), ("compacted", S.contiguous())):
        before = view.clone()
        got = chroma_stft(S=view, sr=CC.SR, tuning=0.0).cpu().numpy()
        mod, _ = CC.model(bank, view.cpu().numpy(), CC.INF, None, np.float32)
        w = CC.worst(got, mod, np.float32)
        print(f"n_fft={n_fft} {name} (strides {tuple(view.stride())}): {w:.3g}")
        assert w <= CC.F32_BAR and torch.equal(view, before)
    # the chained form writes the same padded rows and reads them in place
    monkeypatch.setattr(spectrum, "ROW_ALIGN_BYTES", 128)
    chained = chroma_stft(y=y, sr=CC.SR, tuning=0.0, n_fft=n_fft, hop_length=hop)
    monkeypatch.undo()
    assert torch.equal(chained, chroma_stft(S=S, sr=CC.SR, tuning=0.0)) and torch.equal(chained, chroma_stft(y=y, sr=CC.SR, tuning=0.0, n_fft=n_fft, hop_length=hop))


def test_a_clip_alone_gives_the_bits_of_the_clip_in_a_batch():
    S = CC.stft_s_input("batch3")
    kw = CC.call_kwargs(CC.STFT_S["batch3"]["kw"])
    for A in (np.ascontiguousarray(S), _frame_major(S)):
        whole = chroma_stft(S=A, **kw)
        for i in range(3):
            assert np.array_equal(chroma_stft(S=A[i], **kw), whole[i])
    C = CC.cqt_c_input("batch3")
    kw = CC.call_kwargs(CC.CQT_C["batch3"]["kw"])
    for A in (np.ascontiguousarray(C), _frame_major(C)):
        whole = chroma_cqt(C=A, **kw)
        for i in range(3):
            assert np.array_equal(chroma_cqt(C=A[i], **kw), whole[i])


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("norm", [np.inf, 2, None, 0])
def test_non_finite_input_is_refused_and_leaves_no_flag_behind(bad, norm):
    S = CC.power_spec(91, (2,), 257, 70, np.float32)
    clean = chroma_stft(S=S, sr=CC.SR, tuning=0.0, norm=norm)
    X = S.copy()
    X[1, 200, 69] = bad
    for A in (X, _frame_major(X), _dev(X), _dev(X.swapaxes(-1, -2)).transpose(-1, -2)):
        with pytest.raises(L.ParameterError, match="Input must be finite"):
            chroma_stft(S=A, sr=CC.SR, tuning=0.0, norm=norm)
        assert np.array_equal(chroma_stft(S=S, sr=CC.SR, tuning=0.0, norm=norm), clean)  # the next, clean call
    C = np.abs(S[:, :84])
    C[1, 40, 69] = bad
    for A in (C, _dev(C)):
        with pytest.raises(L.ParameterError, match="Input must be finite"):
            chroma_cqt(C=A, bins_per_octave=12, norm=norm)
    assert np.isfinite(chroma_cqt(C=np.abs(S[:, :84]), bins_per_octave=12, norm=norm)).all()


def test_non_finite_audio_and_overflowing_power():
    y = CC.stft_y_input("y_n512").copy()
    clean = chroma_stft(y=y, sr=CC.SR, tuning=0.0, n_fft=512)
    bad = y.copy()
    bad[3000] = np.inf
    for a in (bad, _dev(bad)):
        with pytest.raises(L.ParameterError, match="Audio buffer is not finite everywhere"):
            chroma_stft(y=a, sr=CC.SR, tuning=0.0, n_fft=512)
    huge = (y * np.float32(1e30)).astype(np.float32)  # finite samples, infinite power: the reference's normalize refuses the chroma
    for a in (huge, _dev(huge)):
        with pytest.raises(L.ParameterError, match="Input must be finite"):
            chroma_stft(y=a, sr=CC.SR, tuning=0.0, n_fft=512)
    assert np.array_equal(chroma_stft(y=y, sr=CC.SR, tuning=0.0, n_fft=512), clean)


@pytest.mark.parametrize("name", list(CC.CQT_C))
def test_chroma_cqt_of_a_transform(golden, name):
    z, _ = golden
    c, C = CC.CQT_C[name], CC.cqt_c_input(name)
    kw = CC.call_kwargs(c["kw"])
    bank = filters.cq_to_chroma(C.shape[-2], **CC.cqt_bank_kwargs(kw))
    out_dtype = CC.result_dtype(C.dtype, bank.dtype)
    mod, _ = CC.model(bank, C, kw.get("norm", CC.INF), kw.get("threshold", 0.0), out_dtype)
    ref = z["out_c_" + name]
    assert ref.dtype == out_dtype and CC.worst(ref, mod, out_dtype) <= CC.bar(out_dtype) / 10
    _both_layouts(lambda A: chroma_cqt(C=A, **kw), C, name, mod, out_dtype)


@pytest.mark.parametrize("name", list(CC.CQT_Y))
def test_chroma_cqt_of_a_signal(golden, monkeypatch, name):
    """cqt -> magnitude -> chroma on the device, with the converter tests/golden/cqt.npz is pinned with on both sides."""
    import cqt_oracle as CQ

    z, _ = golden
    c, y = CC.CQT_Y[name], CC.cqt_y_input(name)
    kw = CC.call_kwargs(c["kw"])
    n_bins, bpo = CC.cqt_dims(kw)
    C64 = np.abs(CQ.cqt(y.astype(np.float64), sr=kw["sr"], n_bins=n_bins, bins_per_octave=bpo, tuning=kw["tuning"], res_type=CC.CQT_RES_TYPE))
    mod, raw = CC.model(filters.cq_to_chroma(n_bins, bins_per_octave=bpo), C64, kw.get("norm", CC.INF), kw.get("threshold", 0.0), np.float32)
    monkeypatch.setattr(chroma_mod, "CQT_RES_TYPE", CC.CQT_RES_TYPE)
    with pytest.warns(UserWarning, match="too large for input signal"):
        got = chroma_cqt(y=y, **kw)
    ref = z["out_" + name]
    assert got.dtype == np.float32 and got.shape == ref.shape
    w = CC.worst(got, mod, np.float32)
    print(f"{name}: {w:.3g} of the frame's maximum; against the reference's result {CC.worst(got, ref.astype(np.float64), np.float32):.3g}")
    assert w <= CC.F32_BAR
    with pytest.warns(UserWarning):
        got_t = chroma_cqt(y=_dev(y), **kw)
    assert got_t.is_cuda and np.array_equal(got_t.cpu().numpy(), got)
    # the unchained form on the device's own transform
    with pytest.warns(UserWarning):
        C = np.abs(L.cqt(y, sr=kw["sr"], n_bins=n_bins, bins_per_octave=bpo, tuning=kw["tuning"], res_type=CC.CQT_RES_TYPE))
    again = chroma_cqt(C=C, **{k: v for k, v in kw.items() if k not in ("sr", "tuning")})
    assert CC.worst(again, mod, np.float32) <= CC.F32_BAR


def test_empty_inputs():
    assert chroma_stft(S=np.zeros((257, 0), np.float32), sr=CC.SR, tuning=0.0).shape == (12, 0)
    assert chroma_stft(S=np.zeros((0, 257, 5), np.float32), sr=CC.SR, tuning=0.0).shape == (0, 12, 5)
    assert chroma_cqt(C=np.zeros((84, 0), np.float64), bins_per_octave=12).dtype == np.float64
