"""chroma_stft / chroma_cqt without a GPU: the two filter banks bit for bit against tests/golden/chroma.npz, every argument error and the
documented "not provided" errors before any device work, and the kernel bodies of librosa_amd/csrc/lra_chroma.h run on the host
(tests/hostsim/chromasim.cpp) in both forms against every fixture case, under the bound of tests/chroma_cases.py."""
import ctypes

import numpy as np
import pytest

import chroma_cases as CC
import hostsim_util
import librosa_amd as L
import stft_oracle as O
from librosa_amd import filters
from librosa_amd.feature import chroma as chroma_mod

chroma_stft, chroma_cqt = L.feature.chroma_stft, L.feature.chroma_cqt

CODES = {None: 0, 1: 1, 2: 2, CC.INF: 3}


@pytest.fixture(scope="module")
def golden():
    return CC.load()


# ---- the tables ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.BANKS))
def test_chroma_bank_is_bit_equal(golden, name):
    _, meta = golden
    kw = CC.bank_kwargs(CC.BANKS[name])
    bank = filters.chroma(**kw)
    assert bank.shape == (kw.get("n_chroma", 12), 1 + kw["n_fft"] // 2) and bank.dtype == kw.get("dtype", np.float32) and bank.flags["C_CONTIGUOUS"]
    assert CC.digest(bank) == meta["banks"][name]
    cached = filters.chroma_cached(**kw)
    assert CC.digest(cached) == meta["banks"][name] and not cached.flags["WRITEABLE"] and filters.chroma_cached(**kw) is cached


@pytest.mark.parametrize("name", list(CC.CQ_BANKS))
def test_cq_to_chroma_bank_is_bit_equal(golden, name):
    _, meta = golden
    n_input, kw = CC.CQ_BANKS[name]
    kw = CC.bank_kwargs(kw)
    want = meta["cq_banks"][name]
    if want == "ParameterError":
        with pytest.raises(L.ParameterError, match="Incompatible CQ merge"):
            filters.cq_to_chroma(n_input, **kw)
        return
    bank = filters.cq_to_chroma(n_input, **kw)
    assert bank.shape == (kw.get("n_chroma", 12), n_input)
    assert CC.digest(bank) == want
    assert CC.digest(filters.cq_to_chroma_cached(n_input, **kw)) == want


def test_the_banks_stored_in_full(golden):
    z, _ = golden
    for got, want in ((filters.chroma(sr=CC.SR, n_fft=64), z["bank_n64"]), (filters.cq_to_chroma(84), z["cq_bank_b12_84"])):
        assert got.dtype == want.dtype and np.array_equal(got, want)


def test_the_chroma_bank_is_dense():
    """Why the banded mel machinery does not apply: every weight is non-zero in float32."""
    bank = filters.chroma(sr=22050, n_fft=2048, tuning=0.0)
    assert np.count_nonzero(bank) == bank.size and bank.min() > 0


@pytest.mark.parametrize("name", list(CC.BANK_ERRORS))
def test_chroma_bank_errors(golden, name):
    _, meta = golden
    assert meta["errors"]["bank_" + name] == "ParameterError"
    with pytest.raises(L.ParameterError, match="Unsupported norm"):
        filters.chroma(**CC.bank_kwargs(CC.BANK_ERRORS[name]))


# ---- argument errors, all before any device work --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.ERRORS))
def test_every_argument_error_of_the_reference(golden, name):
    _, meta = golden
    fn, kw = CC.ERRORS[name]
    assert meta["errors"][name] == "ParameterError"
    kw = {k: (np.zeros(4096, np.float32) if v == "y" else np.ones((84, 4), np.float32) if v == "C84" else v) for k, v in kw.items()}
    with pytest.raises(L.ParameterError):
        getattr(L.feature, fn)(**kw)


def test_not_provided():
    y = np.zeros(4096, np.float32)
    for call in (lambda: chroma_stft(y=y), lambda: chroma_stft(S=np.ones((257, 4), np.float32)), lambda: chroma_stft(y=y, tuning=None), lambda: chroma_cqt(y=y)):
        with pytest.raises(L.ParameterError, match="tuning=None .* not provided"):
            call()
    with pytest.raises(L.ParameterError, match="not provided"):
        chroma_cqt(y=y, tuning=0.0, cqt_mode="hybrid")
    for fn in (L.cqt, L.vqt):  # unchanged
        with pytest.raises(L.ParameterError, match="tuning=None"):
            fn(y, tuning=None)


@pytest.mark.parametrize("norm", [-1, -0.5, "l2", float("nan")])
def test_a_norm_normalize_refuses_is_refused_before_device_work(norm):
    for call in (lambda: chroma_stft(S=np.ones((257, 4), np.float32), tuning=0.0, norm=norm), lambda: chroma_stft(y=np.zeros(4096, np.float32), tuning=0.0, norm=norm),
                 lambda: chroma_cqt(C=np.ones((84, 4), np.float32), norm=norm)):
        with pytest.raises(L.ParameterError, match="Unsupported norm"):
            call()


def test_norm_routing():
    assert [chroma_mod._norm_code(n) for n in (None, 1, 1.0, 2, np.float32(2), np.inf)] == [0, 1, 1, 2, 2, 3]
    assert [chroma_mod._norm_code(n) for n in (0, -np.inf, 3.0, 0.5)] == [None] * 4  # through the host util.normalize
    assert chroma_mod.CQT_RES_TYPE == "soxr_hq"  # the reference's default converter


def test_the_reference_refuses_non_finite_input_for_every_norm(golden):
    _, meta = golden
    assert meta["errors"]["nan_norm_inf"] == meta["errors"]["nan_norm_None"] == "ParameterError: Input must be finite"


def test_complex_and_flat_inputs_are_refused():
    with pytest.raises(L.ParameterError, match="real-valued"):
        chroma_stft(S=np.ones((257, 4), np.complex64), tuning=0.0)
    with pytest.raises(L.ParameterError, match="at least 2 dimensions"):
        chroma_cqt(C=np.ones(84, np.float32))


# ---- the kernel bodies on the host -----------------------------------------------------------------------------------------------------------
_sim = None


def sim_lib():
    global _sim
    if _sim is None:
        _sim = hostsim_util.sim_lib("chromasim", pthread=False)
        c = ctypes
        _sim.chromasim_exec.argtypes = [c.c_void_p] + [c.c_longlong] * 6 + [c.c_int, c.c_void_p, c.c_longlong, c.c_int, c.c_double, c.c_int, c.c_void_p, c.POINTER(c.c_int)]
    return _sim


def sim_run(X, bank, norm, threshold, form, pitch=None):
    """lra_chroma_exec's arguments as feature/chroma.py sets them up.  form "rows": the frame-major layout [b][t][pitch]; "cols": [b][f][t]."""
    lead, (n_bins, n_frames) = X.shape[:-2], X.shape[-2:]
    batch = int(np.prod(lead)) if lead else 1
    real = CC.result_dtype(X.dtype, bank.dtype)
    W = np.ascontiguousarray(bank, dtype=real)
    if form == "rows":
        pitch = n_bins if pitch is None else pitch
        A = np.full((batch, n_frames, pitch), np.nan, real)  # (the padding behind the rows must never be read)
        A[..., :n_bins] = np.swapaxes(X, -1, -2).reshape(batch, n_frames, n_bins)
        strides = (n_frames * pitch, 1, pitch)
    else:
        A = np.ascontiguousarray(X, dtype=real)
        strides = (n_bins * n_frames, n_frames, 1)
    out = np.full((batch, W.shape[0], n_frames), np.nan, real)
    flag = ctypes.c_int(0)
    rc = sim_lib().chromasim_exec(A.ctypes.data, batch, n_bins, n_frames, *strides, int(real == np.float64), W.ctypes.data, W.shape[0], CODES[norm], 0.0 if threshold is None else threshold,
                                  int(threshold is not None), out.ctypes.data, ctypes.byref(flag))
    assert rc == 0
    return out.reshape(lead + out.shape[1:]), bool(flag.value)


def _check(name, X, X64, bank, norm, threshold, ref, pitch=None):
    """Both kernel forms against the model (the norms the kernel does not do: its unnormalised result through the host normalize); the stored
    reference result lies within a tenth of the bound of the same model."""
    device_norm = norm if norm in CODES else None
    out_dtype = CC.result_dtype(X.dtype, bank.dtype)
    mod, _ = CC.model(bank, X64, norm, threshold, out_dtype)
    assert ref.shape == mod.shape and ref.dtype == out_dtype
    assert CC.worst(ref, mod, out_dtype) <= CC.bar(out_dtype) / 10
    for form in ("rows", "cols"):
        got, flagged = sim_run(X, bank, device_norm, threshold, form, pitch if form == "rows" else None)
        assert not flagged and got.dtype == out_dtype
        if device_norm is not norm:
            got = L.util.normalize(got, norm=norm, axis=-2)
        w = CC.worst(got, mod, out_dtype)
        print(f"{name} {form}: {w:.3g} of the frame's maximum")
        assert w <= CC.bar(out_dtype), (name, form, w)


def test_the_case_table_knows_the_kernel_sizes():
    import mel_bank_cases as MB

    lib = sim_lib()
    assert [lib.chromasim_const(i) for i in range(5)] == [CC.FR, CC.PASS, CC.TILE_F, CC.COLS_F, CC.ROWS]
    assert lib.chromasim_const(5) >= 1025 > lib.chromasim_const(6)  # float32 rows of n_fft = 2048 are staged once, float64 rows in two pieces
    assert (CC.F32_BAR, CC.F64_BAR) == (MB.F32_BAR, MB.F64_BAR)
    frames = {c["frames"] for c in CC.STFT_S.values()}
    assert {1, 63, 64, 65} <= frames and any(f % CC.FR and f > CC.TILE_F for f in frames) and any(f % CC.TILE_F and f > 2 * CC.TILE_F for f in frames)
    assert any(f > CC.COLS_F for f in frames) and any(c["kw"].get("n_chroma", 12) > 4 * CC.ROWS for c in CC.STFT_S.values())


@pytest.mark.parametrize("name", list(CC.STFT_S))
def test_sim_chroma_stft_S_cases(golden, name):
    z, meta = golden
    c, S = CC.STFT_S[name], CC.stft_s_input(name)
    assert CC.digest(S) == meta["inputs"]["s_" + name]
    kw = CC.call_kwargs(c["kw"])
    bank = filters.chroma(**CC.stft_bank_kwargs(kw, c["n_fft"]))
    n_bins = S.shape[-2]
    _check(name, S, S.astype(np.float64), bank, kw.get("norm", CC.INF), None, z["out_s_" + name], pitch=n_bins + 7 if name == "n2048_t65" else None)
    if c.get("zero"):
        got, _ = sim_run(S, bank, kw.get("norm", CC.INF), None, "rows")
        assert not np.any(got[1]) and not np.any(got[0][:, c["frames"] // 3 : c["frames"] // 3 + 9]) and np.isfinite(got).all()


@pytest.mark.parametrize("name", list(CC.STFT_Y))
def test_sim_chroma_stft_y_cases(golden, name):
    """The kernels on the oracle's power spectrogram of the signal, rounded to float32 as the device's own is."""
    z, meta = golden
    c, y = CC.STFT_Y[name], CC.stft_y_input(name)
    assert CC.digest(y) == meta["inputs"][name]
    kw = CC.call_kwargs(c["kw"])
    skw = {k: v for k, v in kw.items() if k in ("n_fft", "hop_length", "win_length", "window", "center", "pad_mode")}
    S64 = np.abs(O.stft(y.astype(np.float64), **skw)) ** 2
    bank = filters.chroma(**CC.stft_bank_kwargs(kw, kw["n_fft"]))
    _check(name, S64.astype(np.float32), S64, bank, kw.get("norm", CC.INF), None, z["out_" + name])


@pytest.mark.parametrize("name", list(CC.CQT_C))
def test_sim_chroma_cqt_C_cases(golden, name):
    z, meta = golden
    c, C = CC.CQT_C[name], CC.cqt_c_input(name)
    assert CC.digest(C) == meta["inputs"]["c_" + name]
    kw = CC.call_kwargs(c["kw"])
    bank = filters.cq_to_chroma(C.shape[-2], **CC.cqt_bank_kwargs(kw))
    _check(name, C, C.astype(np.float64), bank, kw.get("norm", CC.INF), kw.get("threshold", 0.0), z["out_c_" + name])


@pytest.mark.parametrize("name", list(CC.CQT_Y))
def test_sim_chroma_cqt_y_cases(golden, name):
    import cqt_oracle as CQ

    z, meta = golden
    c, y = CC.CQT_Y[name], CC.cqt_y_input(name)
    assert CC.digest(y) == meta["inputs"][name]
    kw = CC.call_kwargs(c["kw"])
    n_bins, bpo = CC.cqt_dims(kw)
    C64 = np.abs(CQ.cqt(y.astype(np.float64), sr=kw["sr"], n_bins=n_bins, bins_per_octave=bpo, tuning=kw["tuning"], res_type=CC.CQT_RES_TYPE))
    bank = filters.cq_to_chroma(n_bins, bins_per_octave=bpo)
    _check(name, C64.astype(np.float32), C64, bank, kw.get("norm", CC.INF), kw.get("threshold", 0.0), z["out_" + name])


@pytest.mark.parametrize("form", ["rows", "cols"])
def test_sim_flags_non_finite_values_for_every_norm(form):
    bank = filters.chroma(sr=CC.SR, n_fft=512, n_chroma=36)
    S = CC.power_spec(90, (2,), 257, 70, np.float32)
    for bad in (np.nan, np.inf):
        for norm in (CC.INF, 1, 2, None):
            X = S.copy()
            X[1, 200, 69] = bad
            assert sim_run(X, bank, norm, None, form)[1]
    assert not sim_run(S, bank, CC.INF, None, form)[1]
    # the threshold comes first (chroma[chroma < threshold] = 0 precedes normalize): negative values leave an all-zero, finite array
    C = -CC.cqt_c_input("b12_t65")
    got, flagged = sim_run(C, filters.cq_to_chroma(84), CC.INF, 0.0, form)
    assert not flagged and not np.any(got)
    C[3, 7] = -np.inf  # (times the bank's zeros: NaN in other rows, as in the reference's einsum)
    assert sim_run(C, filters.cq_to_chroma(84), CC.INF, 0.0, form)[1]


def test_sim_a_clip_alone_gives_the_bits_of_the_clip_in_a_batch():
    S = CC.stft_s_input("batch3")
    bank = filters.chroma(sr=CC.SR, n_fft=400)
    for form in ("rows", "cols"):
        whole, _ = sim_run(S, bank, CC.INF, None, form)
        for i in range(3):
            assert np.array_equal(sim_run(S[i], bank, CC.INF, None, form)[0], whole[i])


def test_sim_lengths_below_tiny_are_left_alone():
    bank = filters.cq_to_chroma(84)
    C = np.full((84, 5), 1e-40, np.float32)  # subnormal: every length is below tiny(float32)
    C[:, 2] = 1.0
    for form in ("rows", "cols"):
        got, _ = sim_run(C, bank, CC.INF, None, form)
        raw, _ = sim_run(C, bank, None, None, form)
        assert np.array_equal(got[:, [0, 1, 3, 4]], raw[:, [0, 1, 3, 4]]) and np.all(got[:, 2] == 1.0)
