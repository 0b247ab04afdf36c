"""sequence.viterbi and its variants without a GPU: the golden file against the cases, the NumPy model against the reference, certification, the
transition builders, the argument checks that need no device, the exported names, and the kernel bodies of librosa_amd/csrc/lra_viterbi.h run on
host fibres (tests/hostsim/viterbisim.cpp) behind the package's own Python layer (a session whose buffers are host arrays).

Measured through the simulator: log-domain cases bit-equal; public-path cases at the reference's states with logp off by 0 (float64 prob: the
host's float64 log is NumPy's) and 3.0e-08 (the float32 case), against bounds of 6.3e-13 .. 3.0e-11 and 4.2e-04."""
import ctypes

import numpy as np
import pytest

import hostsim_util
import librosa_amd as L
import viterbi_cases as VC
from librosa_amd import _native
from librosa_amd import sequence as S

_sim = None


def sim_lib():
    global _sim
    if _sim is None:
        _sim = hostsim_util.sim_lib("viterbisim", pthread=False)
        c = ctypes
        _sim.viterbisim_geometry.argtypes = [c.c_int, c.c_int, c.c_void_p]
        _sim.viterbisim_prep.argtypes = [c.c_void_p, c.c_int, c.c_int, c.c_longlong, c.c_int, c.c_longlong, c.c_double, c.c_void_p, c.c_int, c.c_void_p]
        _sim.viterbisim_exec.argtypes = [c.c_void_p, c.c_longlong, c.c_int, c.c_longlong, c.c_void_p, c.c_void_p, c.c_int, c.c_double, c.c_int] + [c.c_void_p] * 6
    return _sim


class SimContext:
    """The two native calls of librosa_amd.sequence, served by the simulator on host pointers."""

    VITERBI_GENERATIVE, VITERBI_DISCRIMINATIVE, VITERBI_BINARY, VITERBI_LOG = (_native.Context.VITERBI_GENERATIVE, _native.Context.VITERBI_DISCRIMINATIVE, _native.Context.VITERBI_BINARY,
                                                                               _native.Context.VITERBI_LOG)
    VITERBI_FLAG_NEGATIVE, VITERBI_FLAG_ABOVE_ONE, VITERBI_FLAG_COLUMN_SUM = (_native.Context.VITERBI_FLAG_NEGATIVE, _native.Context.VITERBI_FLAG_ABOVE_ONE,
                                                                              _native.Context.VITERBI_FLAG_COLUMN_SUM)
    launches = []

    def viterbi_prep_exec(self, prob_ptr, dtype, kind, chains, n_states, n_steps, eps, lm_ptr, n_labels, lp_ptr, work_ptr):
        return sim_lib().viterbisim_prep(prob_ptr, int(np.dtype(dtype) == np.float64), kind, chains, n_states, n_steps, eps, lm_ptr or None, n_labels, lp_ptr)

    def viterbi_exec(self, lp_ptr, chains, n_states, n_steps, lt_ptr, pi_ptr, n_tables, threshold, n_pred, k_ptr, plt_ptr, n_ptr, ptr_ptr, states_ptr, logp_ptr):
        SimContext.launches.append(chains)
        rc = sim_lib().viterbisim_exec(lp_ptr, chains, n_states, n_steps, lt_ptr or None, pi_ptr, n_tables, threshold, n_pred, k_ptr or None, plt_ptr or None, n_ptr or None, ptr_ptr,
                                       states_ptr, logp_ptr)
        assert rc == 0


class SimSession:
    """librosa_amd._arrays.Session with host arrays for buffers; results arrive full of 0xFF bytes: every element must be stored."""

    is_torch = False

    def __init__(self, like):
        self.ctx, self.keep = SimContext(), []

    def input_raw(self, a, dtype):
        a = np.array(a, dtype=dtype, copy=True, order="C")
        self.keep.append(a)
        return a.ctypes.data

    def output(self, shape, dtype, rows=False):
        a = np.frombuffer(bytearray(b"\xff" * max(1, int(np.prod(shape)) * np.dtype(dtype).itemsize)), dtype=dtype)[: int(np.prod(shape))].reshape(shape)
        self.keep.append(a)
        return a.ctypes.data, a

    def result(self, handle):
        return handle

    def scratch(self, nbytes):
        a = np.empty(max(int(nbytes), 16), np.uint8)
        self.keep.append(a)
        return a.ctypes.data

    def close(self):
        pass


@pytest.fixture
def on_sim(monkeypatch):
    monkeypatch.setattr(S._arrays, "Session", SimSession)
    SimContext.launches = []
    return SimContext


FNS = VC.functions(S)


run_case, check_case = VC.run_case, VC.check_case


# ---- the golden file, the model, certification ------------------------------------------------------------------------------------------------
def test_golden_covers_the_cases():
    arrays, meta = VC.load()
    assert set(meta["cases"]) == set(VC.CASES)
    for name in VC.CASES:
        st, lp = arrays[f"{name}/states"], arrays[f"{name}/logp"]
        assert st.dtype == np.uint16 and lp.dtype == np.float64
        assert (st.shape, lp.shape) == VC.out_shapes(name), name
    assert set(meta["refusals"]) == set(VC.refusals()) and set(meta["builder_errors"]) == set(VC.BUILDER_ERRORS)
    # the shapes the issue pins: (1,) for the 2-D generative call, a scalar for the discriminative one
    assert arrays["v_s3/logp"].shape == (1,) and arrays["d_s3_thr/logp"].shape == () and arrays["b_1d/states"].shape == (1, 10)


@pytest.mark.parametrize("name", list(VC.CASES))
def test_model_matches_the_reference_and_case_is_certified(name):
    arrays, meta = VC.load()
    states, logp, margin = VC.model_case(name)
    assert np.array_equal(states.reshape(arrays[f"{name}/states"].shape), arrays[f"{name}/states"])
    assert np.array_equal(logp.reshape(arrays[f"{name}/logp"].shape), arrays[f"{name}/logp"], equal_nan=True)
    if VC.CASES[name]["fn"] != "log":
        d = VC.delta(name, arrays[f"{name}/logp"])
        assert d == meta["cases"][name]["delta"] and margin == (np.inf if meta["cases"][name]["margin"] is None else meta["cases"][name]["margin"])
        assert margin >= VC.MARGIN_FLOOR and margin >= VC.MARGIN_FACTOR * d, f"{name}: margin {margin:.3g}, delta {d:.3g}: change the seed"


def test_max_states_case_dense_and_sparse_forms_agree():
    k, v, n = VC.band_lists(64)
    dense = VC.band_dense(64)
    pk, plt, pn = S._predecessors(dense, -20.0)
    assert np.array_equal(pk, k) and np.array_equal(plt, v) and np.array_equal(pn, n)


# ---- the builders -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VC.BUILDERS))
def test_transition_builder_equals_the_reference(name):
    fn, args, kw = VC.BUILDERS[name]
    got, want = getattr(S, fn)(*args, **kw), VC.load()[0][f"builder/{name}"]
    assert got.dtype == np.float64 and np.array_equal(got, want)


@pytest.mark.parametrize("name", list(VC.BUILDER_ERRORS))
def test_transition_builder_refuses_as_the_reference(name):
    fn, args, kw = VC.BUILDER_ERRORS[name]
    with pytest.raises(L.ParameterError) as e:
        getattr(S, fn)(*args, **kw)
    assert str(e.value) == VC.load()[1]["builder_errors"][name]


# ---- argument checks --------------------------------------------------------------------------------------------------------------------------
class NoDevice:
    def __init__(self, like):
        raise AssertionError("the call reached the device")


@pytest.mark.parametrize("name", [n for n, r in VC.refusals().items() if not r[4]])
def test_refused_without_a_device(name, monkeypatch):
    monkeypatch.setattr(S._arrays, "Session", NoDevice)
    fn, prob, transition, kw, _ = VC.refusals()[name]
    with pytest.raises(L.ParameterError) as e:
        getattr(S, fn)(prob, transition, **kw)
    assert str(e.value) == VC.load()[1]["refusals"][name]


@pytest.mark.parametrize("name", [n for n, r in VC.refusals().items() if r[4]])
def test_prob_range_flags_refuse_before_the_decode(name, on_sim):
    fn, prob, transition, kw, _ = VC.refusals()[name]
    with pytest.raises(L.ParameterError) as e:
        getattr(S, fn)(prob, transition, **kw)
    assert str(e.value) == VC.load()[1]["refusals"][name]
    assert on_sim.launches == []


def test_one_state_above_the_limit_is_refused_before_device_work(monkeypatch):
    monkeypatch.setattr(S._arrays, "Session", NoDevice)
    n = VC.MAX_STATES + 1
    assert S.MAX_STATES == VC.MAX_STATES
    table = np.broadcast_to(np.float32(0), (n, n))   # (no memory behind it: the limit is checked before the table is read)
    for call in (lambda: S.viterbi(np.zeros((n, 2)), table), lambda: S.viterbi_discriminative(np.zeros((n, 2)), table),
                 lambda: S._viterbi_log(np.zeros((n, 2)), table, np.zeros(n), -np.inf)):
        with pytest.raises(L.ParameterError, match=f"n_states={n} is too large"):
            call()
    lib = _native.load_library()
    assert lib.lra_viterbi_lds_bytes(VC.MAX_STATES, 0) <= 160 * 1024 < lib.lra_viterbi_lds_bytes(n, 0)
    assert lib.lra_viterbi_lds_bytes(VC.MAX_STATES, 5) <= 160 * 1024


def test_exported_names():
    assert "sequence" in L.__all__ and L.sequence is S
    for name in ("viterbi", "viterbi_discriminative", "viterbi_binary", "transition_uniform", "transition_loop", "transition_cycle", "transition_local"):
        assert name in S.__all__ and callable(getattr(S, name))
    assert callable(S._viterbi_log)


# ---- the kernel bodies on host fibres -----------------------------------------------------------------------------------------------------------
def geometry(n_states, n_pred=0):
    out = np.zeros(5, np.int32)
    sim_lib().viterbisim_geometry(n_states, n_pred, out.ctypes.data_as(ctypes.c_void_p))
    return dict(small=int(out[0]), nt=int(out[1]), lanes=int(out[2]), table_lds=int(out[3]), lds=int(out[4]))


def test_launch_geometry():
    assert geometry(VC.SMALL_MAX)["small"] == 1 and geometry(VC.SMALL_MAX + 1)["small"] == 0
    assert geometry(2)["lanes"] == 2 and 256 // geometry(2)["lanes"] == VC.SMALL_CHAINS and geometry(3)["lanes"] == 4 and geometry(32)["lanes"] == 32
    assert geometry(33) == dict(small=0, nt=256, lanes=4, table_lds=1, lds=16 * 33 + 12 * 256 + 8 * 33 * 33)
    assert geometry(64)["lanes"] == 4 and geometry(65)["lanes"] == 2 and geometry(128)["lanes"] == 2 and geometry(129)["lanes"] == 1
    assert geometry(70, 1)["lanes"] == 1 and geometry(70, 3)["lanes"] == 2
    assert geometry(141)["table_lds"] == 1 and geometry(142)["table_lds"] == 0 and geometry(100, 7)["table_lds"] == 0
    assert geometry(1024)["nt"] == 1024 and geometry(1025)["nt"] == 576 and geometry(1200, 160) == dict(small=0, nt=640, lanes=1, table_lds=0, lds=16 * 1200 + 12 * 640)
    for s in (1, 32, 33, 141, 142, 1025, VC.MAX_STATES):
        for p in (0, 5):
            g = geometry(s, p)
            assert g["lds"] <= 160 * 1024 and g["nt"] % 64 == 0 and g["nt"] <= 1024
            assert g["lds"] == _native.load_library().lra_viterbi_lds_bytes(s, p)


worst = {}


@pytest.mark.parametrize("name", list(VC.CASES))
def test_kernel_bodies_on_the_host(name, on_sim):
    states, logp = run_case(name, S)
    worst[name] = check_case(name, np.asarray(states), np.asarray(logp), report=print)
    assert len(on_sim.launches) == 1   # one launch over every sequence and label


def test_batch_equals_per_item_and_chunks_on_the_host(on_sim, monkeypatch):
    for name in ("d_lead23", "v_lead23_thr", "b_tables70", "log_ties_small"):
        c, a = VC.CASES[name], VC.inputs(name)
        whole = run_case(name, S)
        if c["fn"] == "log":
            items = [S._viterbi_log(x, a["log_trans"], a["log_p_init"], a["thr"]) for x in a["log_prob"]]
        else:
            items = [FNS[c["fn"]](x, a["transition"], return_logp=True, **a["kw"]) for x in a["prob"].reshape((-1,) + a["prob"].shape[len(c["lead"]):])]
        assert np.array_equal(np.stack([i[0] for i in items]).reshape(whole[0].shape), whole[0])
        assert np.array_equal(np.stack([i[1] for i in items]).reshape(whole[1].shape), whole[1])
        # a scratch budget of two sequences (binary: of one item's labels): the same bits from several launches
        on_sim.launches.clear()
        monkeypatch.setattr(S, "SCRATCH_BUDGET", 10 * 2 * c["T"] * c["S"])
        chunked = run_case(name, S)
        assert len(on_sim.launches) > 1
        assert np.array_equal(chunked[0], whole[0]) and np.array_equal(chunked[1], whole[1])
        monkeypatch.undo()
        monkeypatch.setattr(S._arrays, "Session", SimSession)
