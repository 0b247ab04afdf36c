"""tempogram / tempo without a GPU: argument checks before any device work, the host tables against tests/golden/rhythm.npz, and the kernel
bodies of librosa_amd/csrc/lra_rhythm.h run on host threads (tests/hostsim/rhythmsim.cpp) on the reference's envelopes."""
import ctypes

import numpy as np
import pytest

import hostsim_util
import librosa_amd as L
import rhythm_cases as RC
from librosa_amd.feature import rhythm as R


@pytest.fixture(scope="module")
def golden():
    return RC.load()


# ---- argument checks: ParameterError before any device call (this host has no GPU: a device call would raise NativeError) ----------------
def test_win_length_must_be_positive():
    env = np.ones(100, np.float32)
    for f in (L.feature.tempogram, L.feature.fourier_tempogram):
        with pytest.raises(L.ParameterError):
            f(onset_envelope=env, win_length=0)
    with pytest.raises(L.ParameterError):  # ac_size * sr < hop_length: a window of no frames
        L.feature.tempo(onset_envelope=env, ac_size=0.01)


def test_window_array_must_have_win_length():
    with pytest.raises(L.ParameterError):
        L.feature.tempogram(onset_envelope=np.ones(100, np.float32), win_length=64, window=np.ones(63))


def test_an_input_is_required():
    with pytest.raises(L.ParameterError):
        L.feature.tempogram()
    with pytest.raises(L.ParameterError):
        L.feature.fourier_tempogram()
    with pytest.raises(L.ParameterError):
        L.feature.tempo()


def test_start_bpm_must_be_positive():
    for bpm in (0, -10):
        with pytest.raises(L.ParameterError):
            L.feature.tempo(onset_envelope=np.ones(100, np.float32), start_bpm=bpm)


def test_short_envelope_without_centring_is_rejected():
    with pytest.raises(L.ParameterError):
        L.feature.tempogram(onset_envelope=np.ones(100, np.float32), win_length=101, center=False)
    with pytest.raises(L.ParameterError):  # odd window, empty envelope: W // 2 on each side is one short
        L.feature.tempogram(onset_envelope=np.ones(0, np.float32), win_length=7)
    with pytest.raises(L.ParameterError):  # from y: the envelope's length is known before the mel is computed
        L.feature.tempogram(y=np.zeros(4096, np.float32), win_length=64, center=False)


def test_norm_codes():
    assert R._norm_code(np.inf) == R._NORM_INF and R._norm_code(None) == R._NORM_NONE
    assert R._norm_code(1) == R._NORM_L1 and R._norm_code(2.0) == R._NORM_L2
    for host in (3, -np.inf, 0, 0.5, True, "x"):
        assert R._norm_code(host) is None


# ---- the host tables --------------------------------------------------------------------------------------------------------------------
def test_frequency_tables_match_the_reference(golden):
    z, _, _ = golden
    for W, hop, sr in ((384, 512, 22050), (344, 512, 22050), (800, 160, 16000), (8, 441, 22050)):
        np.testing.assert_array_equal(L.tempo_frequencies(W, hop_length=hop, sr=sr), z[f"tempo_frequencies_{W}_{hop}_{sr}"])
        np.testing.assert_array_equal(L.fourier_tempo_frequencies(sr=sr, win_length=W, hop_length=hop), z[f"fourier_tempo_frequencies_{W}_{hop}_{sr}"])
    assert L.core.tempo_frequencies is L.tempo_frequencies


@pytest.mark.parametrize("name", RC.names("tempo"))
def test_bpm_and_prior_tables_are_bit_equal(golden, name):
    z, cases, inputs = golden
    call = RC.call_kwargs(cases[name]["kwargs"], inputs)
    sr, hop = call.get("sr", RC.SR), call.get("hop_length", 512)
    W = 384 if cases[name]["input"].startswith("tg:") else int(8.0 * sr) // hop  # tg given: its own window (tempogram's default here)
    bpms, lp = R._tables(W, hop, sr, call.get("start_bpm", 120), call.get("std_bpm", 1.0), call.get("max_tempo", 320.0), call.get("prior"))
    np.testing.assert_array_equal(bpms, z[f"bpms_{name}"])
    np.testing.assert_array_equal(lp, z[f"logprior_{name}"])


# ---- the kernel bodies on host threads --------------------------------------------------------------------------------------------------
_sim = None


def sim_lib():
    global _sim
    if _sim is None:
        _sim = hostsim_util.sim_lib("rhythmsim", pthread=True)
        c = ctypes
        _sim.rhythmsim_exec.argtypes = [c.c_void_p, c.c_longlong, c.c_longlong, c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_int, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p,
                                        c.c_int, c.POINTER(c.c_int)]
    return _sim


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def sim_exec(env, W, center, window, norm, mode, logprior=None, bpms=None, direct=False):
    """One lra_tempogram_exec through the simulator on (..., n) envelopes; the output arrives full of NaN: every element must be stored."""
    env = np.ascontiguousarray(env)
    lead, n = env.shape[:-1], env.shape[-1]
    batch = int(np.prod(lead)) if lead else 1
    nf = n if center else n - W + 1
    shape = {R._WRITE: (batch, W, nf), R._SUM: (batch, 1), R._ARGMAX: (batch, nf)}[mode]
    out = np.full(shape, np.nan)
    flag = ctypes.c_int(0)
    win = np.ascontiguousarray(window, dtype=np.float64)
    rc = sim_lib().rhythmsim_exec(_p(env), batch, n, int(env.dtype == np.float64), W, int(center), _p(win), norm, mode, _p(logprior), _p(bpms), _p(out), int(direct), ctypes.byref(flag))
    assert rc == 0
    return out.reshape(lead + shape[1:]), bool(flag.value)


def test_transform_lengths_are_the_restated_ones():
    """The library's own choice of transform (lra_rhythm.h: prepare, through the simulator) against tests/rhythm_edges.py's restatement: at, one below
    and one above the largest window of every size, where the choice changes; and the tile and the LDS total that go with it."""
    import rhythm_edges as E

    sim_lib().rhythmsim_geometry.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    for N in E.SIZES:
        for W in ((N + 1) // 2 - 1, (N + 1) // 2, (N + 1) // 2 + 1):
            for mode in (R._WRITE, R._SUM, R._ARGMAX):
                out = np.zeros(3, np.int32)
                sim_lib().rhythmsim_geometry(W, mode, _p(out))
                tile = mode == R._WRITE and E.lds_total(W, mode, True) <= E.LDS_MAX
                assert (int(out[0]), bool(out[1]), int(out[2])) == (E.transform_length(W), tile, E.lds_total(W, mode, tile)), (N, W, mode)
    assert E.transform_length((E.SIZES[-1] + 1) // 2 + 1) == 0  # the sweep ends on the direct kernel


def _envelope_case(z, cases, inputs, name):
    call = RC.call_kwargs(cases[name]["kwargs"], inputs)
    W = call.get("win_length", 384)
    window = L.filters.get_window(call.get("window", "hann"), W, fftbins=True)
    return z[f"env_{name}"], W, call.get("center", True), window, call.get("norm", np.inf)


SIM_TEMPOGRAMS = ["tg_env_1d", "tg_env_3d", "tg_w344", "tg_w127", "tg_w8", "tg_nocenter", "tg_norm_none", "tg_norm_1", "tg_norm_2", "tg_win_ones", "tg_win_array", "tg_zero",
                  "tg_short"]


@pytest.mark.parametrize("name", SIM_TEMPOGRAMS)
def test_simulated_tempogram_matches_the_reference(golden, name):
    z, cases, inputs = golden
    env, W, center, window, norm = _envelope_case(z, cases, inputs, name)
    got, bad = sim_exec(env, W, center, window, R._norm_code(norm), R._WRITE)
    assert not bad and not np.isnan(got).any()
    assert got.dtype == np.float64 and got.shape == z[f"env_{name}"].shape[:-1] + (W, env.shape[-1] if center else env.shape[-1] - W + 1)
    assert RC.col_err(RC.sampled(z, name, got), z[name]) <= 1e-13


def test_direct_kernel_matches_the_transform():
    rng = np.random.default_rng(3)
    env = np.abs(rng.standard_normal((2, 40))).astype(np.float32)
    for W, norm in ((37, R._NORM_INF), (64, R._NORM_L2)):
        win = L.filters.get_window("hann", W, fftbins=True)
        a, _ = sim_exec(env, W, True, win, norm, R._WRITE)
        b, _ = sim_exec(env, W, True, win, norm, R._WRITE, direct=True)
        assert RC.col_err(b, a) <= 1e-13


def test_simulated_nonfinite_envelope_sets_the_flag():
    env = np.ones(50, np.float32)
    env[20] = np.nan
    for norm in (R._NORM_NONE, R._NORM_INF):
        _, bad = sim_exec(env, 16, True, np.hanning(16), norm, R._WRITE)
        assert bad


@pytest.mark.parametrize("name", ["tempo_env", "tempo_y", "tempo_pulses", "tempo_16k", "tempo_silent", "tempo_none"])
def test_simulated_tempo_matches_the_reference(golden, name):
    z, cases, inputs = golden
    env = z[f"env_{name}"]
    bpms, lp = z[f"bpms_{name}"], z[f"logprior_{name}"]
    W = len(bpms)
    mode = R._ARGMAX if name == "tempo_none" else R._SUM
    got, bad = sim_exec(env, W, True, L.filters.get_window("hann", W, fftbins=True), R._NORM_INF, mode, lp, bpms)
    assert not bad
    want, margin = z[name], z[f"margin_{name}"]
    got = got.reshape(want.shape)
    ok = margin.reshape(want.shape) >= 1e-9  # from the reference's own envelope: float64 rounding only
    assert ok.mean() >= 0.9
    np.testing.assert_array_equal(got[ok], want[ok])
    if mode == R._SUM:  # the same clip alone gives the same bits
        one, _ = sim_exec(env.reshape(-1, env.shape[-1])[-1], W, True, L.filters.get_window("hann", W, fftbins=True), R._NORM_INF, mode, lp, bpms)
        assert one.reshape(-1)[0] == got.reshape(-1)[-1]
