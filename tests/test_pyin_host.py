"""pyin without a GPU: the golden file against the cases, the NumPy model against the reference's ``__pyin_helper``, the certification figures, the
refusals before any device work, the exported names, and the kernel bodies of librosa_amd/csrc/lra_pyin.h run on host fibres
(tests/hostsim/pyinsim.cpp) behind the package's own Python layer (a session whose buffers are host arrays; the front half and the decode run
through yinsim and viterbisim in the same way).

Parts (a), (b) and (d) of tests/pyin_cases.py.  Measured through the simulator, worst over the cases of (a): a voiced entry 7.1e-15 from
log(p_ref + tiny) (0.19 of its bound); voiced_prob 2.2e-16 from the reference's (bound 5.1e-14); an unvoiced probability 6.9e-18 off
(0.005 of its bound).  (b): every state count bit-equal for every fill_na."""
import ctypes
import os

import numpy as np
import pytest

import hostsim_util
import librosa_amd as L
import pyin_cases as PC
import test_viterbi_host as TV
import test_yin_host as TY
from librosa_amd import _native
from librosa_amd import sequence as S
from librosa_amd.core import pitch as P

_sim = None


def sim_lib():
    global _sim
    if _sim is None:
        _sim = hostsim_util.sim_lib("pyinsim", pthread=False)
        c = ctypes
        _sim.pyinsim_geometry.argtypes = [c.c_int, c.c_int, c.c_void_p]
        _sim.pyinsim_obs.argtypes = [c.c_void_p, c.c_void_p, c.c_longlong, c.c_int, c.c_longlong] + [c.c_void_p] * 5 + [c.c_int, c.c_double, c.c_double, c.c_int, c.c_int, c.c_int, c.c_double,
                                                                                                                          c.c_double, c.c_double, c.c_void_p, c.c_void_p]
        _sim.pyinsim_finish.argtypes = [c.c_void_p, c.c_longlong, c.c_int, c.c_void_p, c.c_int, c.c_double, c.c_void_p, c.c_void_p]
    return _sim


class SimContext(TV.SimContext):
    """The native calls of pyin's pipeline, served by the simulators on host pointers."""

    obs_launches = []

    def yin_exec(self, y_ptr, batch, n, dtype, frame_length, hop_length, center, pad_mode, min_period, max_period, trough_threshold, sr, mode, f0_ptr=0, frames_ptr=0, shifts_ptr=0):
        rc = TY.sim_lib().yinsim_exec(y_ptr, batch, n, int(np.dtype(dtype) == np.float64), frame_length, hop_length, int(center), TY.PAD_MODES[pad_mode], min_period, max_period,
                                      float(trough_threshold), float(sr), mode, f0_ptr or None, frames_ptr or None, shifts_ptr or None, 0)
        assert rc == 0

    def pyin_obs_exec(self, cm_ptr, sh_ptr, clips, n_lags, n_frames, thr_ptr, beta_ptr, prefix_ptr, e_ptr, fact_ptr, n_thresholds, sr, fmin, min_period, n_pitch_bins, n_bins_per_semitone,
                      no_trough_prob, tiny, log_tiny, lp_ptr, vp_ptr):
        SimContext.obs_launches.append(clips)
        rc = sim_lib().pyinsim_obs(cm_ptr, sh_ptr, clips, n_lags, n_frames, thr_ptr, beta_ptr, prefix_ptr, e_ptr, fact_ptr, n_thresholds, sr, fmin, min_period, n_pitch_bins, n_bins_per_semitone,
                                   no_trough_prob, tiny, log_tiny, lp_ptr, vp_ptr)
        assert rc == 0

    def pyin_finish_exec(self, states_ptr, n, n_pitch_bins, freqs_ptr, fill_na, f0_ptr, voiced_ptr):
        assert sim_lib().pyinsim_finish(states_ptr, n, n_pitch_bins, freqs_ptr, int(fill_na is not None), 0.0 if fill_na is None else float(fill_na), f0_ptr, voiced_ptr) == 0


class SimSession(TV.SimSession):
    def __init__(self, like):
        self.ctx, self.keep = SimContext(), []

    def output(self, shape, dtype, rows=False):
        if int(np.prod(shape)) == 0:   # (an empty batch)
            a = np.empty(shape, dtype=dtype)
            self.keep.append(a)
            return a.ctypes.data, a
        return super().output(shape, dtype, rows)

    def input_2d(self, x, dtype):
        a = np.array(x, dtype=dtype, copy=True, order="C").reshape(-1, x.shape[-1])
        self.keep.append(a)
        return a.ctypes.data, a.shape[0], a.shape[1], a.shape[1]


@pytest.fixture
def on_sim(monkeypatch):
    monkeypatch.setattr(S._arrays, "Session", SimSession)
    SimContext.launches = []
    SimContext.obs_launches = []
    return SimContext


@pytest.fixture(scope="module")
def golden():
    return PC.load()


class NoDevice:
    def __init__(self, like):
        raise AssertionError("the call reached the device")


# ---- the golden file, the model, certification ------------------------------------------------------------------------------------------------
def test_golden_covers_the_cases(golden):
    arrays, meta = golden
    assert set(meta["obs"]) == set(PC.OBS_CASES) and set(meta["e2e"]) == set(PC.E2E_CASES) and set(meta["refusals"]) == set(PC.refusal_calls())
    assert os.path.getsize(PC.GOLDEN) < 1 << 20
    assert meta["synthetic"] == PC.digest(PC.synthetic_rows())
    for name in PC.OBS_CASES:
        cm, sh = PC.obs_inputs(name, arrays)
        assert meta["obs"][name]["cmnd"] == PC.digest(cm) and meta["obs"][name]["shifts"] == PC.digest(sh), name
    for name in PC.E2E_CASES:
        assert meta["e2e"][name]["y"] == PC.digest(PC.e2e_signal(name)), name
        assert meta["e2e"][name]["states"] == PC.e2e_states(name)
        assert ("eobs_" + name in arrays) == (meta["e2e"][name]["states"] <= 242)
    assert {c["states"] for c in PC.GLUE_CASES.values()} == {24, 50, 242, 1202} and meta["e2e"]["e_default"]["states"] == 1202


@pytest.mark.parametrize("name", list(PC.OBS_CASES))
def test_model_matches_the_reference_and_every_candidate_is_settled(golden, name):
    arrays, meta = golden
    cm, sh = PC.obs_inputs(name, arrays)
    p_mod, vp_mod, info = PC.obs_model(cm, sh, PC.obs_kw(name))
    P_ = meta["obs"][name]["P"]
    want = arrays["obs_" + name]
    assert np.array_equal(p_mod[..., :P_, :] == 0, want == 0) and np.allclose(p_mod[..., :P_, :], want, rtol=1e-13, atol=0)
    assert np.allclose(vp_mod, arrays["vp_" + name], rtol=0, atol=1e-13)
    assert info["half"] > PC.HALF_MARGIN, f"{name}: a candidate {info['half']:.3g} from a half: change the seed"
    assert sorted(info["events"]) == meta["obs"][name]["events"]


def test_synthetic_rows_meet_every_event(golden):
    _, meta = golden
    assert set(meta["obs"]["syn"]["events"]) | set(meta["obs"]["syn_r05"]["events"]) >= PC.SYN_EVENTS
    assert "two_in_one_bin" in meta["obs"]["noise64_r05"]["events"]


def test_end_to_end_cases_are_certified(golden):
    _, meta = golden
    for name, m in meta["e2e"].items():
        assert m["margin"] > PC.CERT_FACTOR * m["delta"] and m["half"] > PC.HALF_MARGIN + 1e4 * PC.CERT_FACTOR * m["delta"], name
    assert meta["e2e"]["e_zeros"]["voiced"] == 0 and meta["e2e"]["e_one_frame"]["frames"] == 1


# ---- (d) refusals, names ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.refusal_calls()))
def test_refused_before_device_work(golden, name, monkeypatch):
    monkeypatch.setattr(S._arrays, "Session", NoDevice)
    PC.check_refusal(name, L, golden[1])


def test_private_entry_refuses_the_same_limits(monkeypatch):
    monkeypatch.setattr(S._arrays, "Session", NoDevice)
    cm = np.ones((4, 3))
    with pytest.raises(L.ParameterError, match="too large for the device decoder"):
        P._pyin_log_prob(cm, cm, sr=22050, fmin=PC.C2, fmax=PC.C7, min_period=10, resolution=0.01)
    with pytest.raises(L.ParameterError, match="positive integer"):
        P._pyin_log_prob(cm, cm, sr=22050, fmin=100.0, fmax=200.0, min_period=10, n_thresholds=True)
    with pytest.raises(L.ParameterError, match="too large for the device"):
        P._pyin_log_prob(cm, cm, sr=22050, fmin=100.0, fmax=200.0, min_period=10, n_thresholds=30000)


def test_names_are_exported():
    assert L.pyin is L.core.pyin is P.pyin
    assert "pyin" in L.__all__ and "pyin" in L.core.__all__ and "pyin" in P.__all__
    assert callable(P._pyin_log_prob)
    for name in ("lra_pyin_lds_bytes", "lra_pyin_obs_exec", "lra_pyin_finish_exec"):
        assert name in _native.SIGNATURES
    from librosa_amd import build

    assert "pyin_inst" in build.UNITS


def test_bounds_are_keyword_only_and_required():
    with pytest.raises(TypeError):
        L.pyin(np.ones(4096))
    with pytest.raises(TypeError):
        L.pyin(np.ones(4096), 100.0, 2000.0)


# ---- the kernel bodies on host fibres -----------------------------------------------------------------------------------------------------------
def geometry(n_pitch_bins, n_thresholds):
    out = np.zeros(2, np.int32)
    sim_lib().pyinsim_geometry(n_pitch_bins, n_thresholds, out.ctypes.data_as(ctypes.c_void_p))
    return dict(waves=int(out[0]), lds=int(out[1]))


def test_launch_geometry_is_the_librarys():
    lib = _native.load_library()
    assert geometry(601, 100) == dict(waves=4, lds=4 * (8 * 601 + 800))
    assert geometry(4096, 100)["waves"] == 4 and geometry(4096, 2000)["waves"] == 2 and geometry(4096, 10000)["waves"] == 1
    for P_, n in ((12, 1), (601, 100), (4096, 100), (4096, 2000), (4096, 10000), (4096, 16384)):
        assert lib.lra_pyin_lds_bytes(P_, n) == geometry(P_, n)["lds"] <= 160 * 1024
    assert lib.lra_pyin_lds_bytes(4096, 16385) > 160 * 1024


worst = {}


@pytest.mark.parametrize("name", list(PC.OBS_CASES))
def test_observation_kernel_on_the_host(golden, name, on_sim):
    worst[name] = PC.run_obs_case(name, P, golden[0], report=print)
    assert len(on_sim.obs_launches) == 1


def test_a_clip_gives_the_same_bits_alone_and_in_a_batch(golden, on_sim):
    cm, sh = PC.obs_inputs("noise_lead23", golden[0])
    p = PC.obs_params(PC.obs_kw("noise_lead23"))[0]
    whole = P._pyin_log_prob(cm, sh, **p)
    one = P._pyin_log_prob(cm[1, 2], sh[1, 2], **p)
    assert np.array_equal(whole[0][1, 2], one[0]) and np.array_equal(whole[1][1, 2], one[1])


@pytest.mark.parametrize("name,tmp", [(n, t) for n, c in PC.GLUE_CASES.items() for t in ((1e-4, None) if c["none"] else (1e-4,))])
def test_decode_glue_on_the_host(name, tmp, on_sim):
    voiced, frames = PC.run_glue_case(name, L, tmp)
    assert 0 < voiced < frames, (voiced, frames)   # both halves of the state space are met


def test_chunks_give_the_same_bits_on_the_host(golden, on_sim, monkeypatch):
    c = PC.E2E_CASES["e_lead23"]
    y = PC.e2e_signal("e_lead23")
    whole = L.pyin(y, **c["kw"])
    assert on_sim.obs_launches == [6]
    for got, key in zip(whole, ("f0_", "flag_", "vp_")):
        assert got.shape == golden[0][key + "e_lead23"].shape
    one = L.pyin(y[1, 2], **c["kw"])
    on_sim.obs_launches.clear()
    n_lags, n_frames = 74 - 36 + 1, whole[0].shape[-1]
    monkeypatch.setattr(S, "SCRATCH_BUDGET", 2 * (16 * n_lags + 10 * 242) * n_frames)
    chunked = L.pyin(y, **c["kw"])
    assert on_sim.obs_launches == [2, 2, 2]
    for a, b, o in zip(whole, chunked, one):
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a[1, 2], o, equal_nan=True)


def test_an_empty_batch_gives_empty_results(on_sim):
    f0, flag, vp = L.pyin(np.zeros((0, 1000)), **PC.E2E_CASES["e_noise"]["kw"])
    n_frames = 1 + 1000 // 64
    assert f0.shape == flag.shape == vp.shape == (0, n_frames) and (f0.dtype, flag.dtype, vp.dtype) == (np.float64, np.bool_, np.float64)
