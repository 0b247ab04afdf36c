"""sequence.dtw and dtw_backtracking without a GPU: the golden file against the cases, the NumPy model against the golden, the argument checks
that need no device, the documented differences, the exported names, and the kernel bodies of librosa_amd/csrc/lra_dtw.h run on host fibres
(tests/hostsim/dtwsim.cpp) behind the package's own Python layer (a session whose buffers are host arrays, results full of 0xFF bytes).

Measured through the simulator: every ``C=`` case and every ``dtw_backtracking`` case bit-equal; every X/Y case at the reference's path with D
off by at most 1.6e-14 (the two cosine cases; every other case 0), against bounds of 4.9e-13 .. 6.4e-11."""
import ctypes
import os
import re

import numpy as np
import pytest

import dtw_cases as DC
import hostsim_util
import librosa_amd as L
from librosa_amd import _native
from librosa_amd import sequence as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_sim = None


def sim_lib():
    global _sim
    if _sim is None:
        _sim = hostsim_util.sim_lib("dtwsim", pthread=False)
        c = ctypes
        _sim.dtwsim_geometry.argtypes = [c.c_int, c.c_int, c.c_int, c.c_void_p]
        _sim.dtwsim_cost.argtypes = [c.c_void_p, c.c_void_p, c.c_int, c.c_longlong, c.c_longlong, c.c_longlong, c.c_int, c.c_void_p]
        _sim.dtwsim_prepare.argtypes = [c.c_void_p, c.c_int, c.c_longlong, c.c_void_p]
        _sim.dtwsim_accumulate.argtypes = [c.c_void_p, c.c_longlong, c.c_longlong, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_longlong, c.c_longlong, c.c_int, c.c_void_p,
                                           c.c_void_p]
        _sim.dtwsim_accumulate.restype = c.c_longlong
        _sim.dtwsim_widen.argtypes = [c.c_void_p, c.c_longlong, c.c_void_p]
        _sim.dtwsim_backtrack.argtypes = [c.c_void_p, c.c_void_p, c.c_int, c.c_longlong, c.c_longlong, c.c_void_p, c.c_int, c.c_int, c.c_longlong, c.c_void_p, c.c_void_p]
    return _sim


class SimContext:
    """The native calls of librosa_amd.sequence's DTW, served by the simulator on host pointers."""

    DTW_METRICS, DTW_TYPES = _native.Context.DTW_METRICS, _native.Context.DTW_TYPES
    DTW_FLAG_NAN, DTW_FLAG_END_INF, DTW_FLAG_ROW_INF, DTW_FLAG_NOT_ORIGIN, DTW_FLAG_BAD_STEP = (_native.Context.DTW_FLAG_NAN, _native.Context.DTW_FLAG_END_INF, _native.Context.DTW_FLAG_ROW_INF,
                                                                                               _native.Context.DTW_FLAG_NOT_ORIGIN, _native.Context.DTW_FLAG_BAD_STEP)
    DTW_START_END, DTW_START_ARGMIN = _native.Context.DTW_START_END, _native.Context.DTW_START_ARGMIN
    launches = []   # per accumulate call: the number of kernel launches
    calls = []      # the native calls made, by name

    def dtw_cost_exec(self, x_ptr, y_ptr, dtype, n_features, n, m, metric, c_ptr, work_ptr):
        SimContext.calls.append("cost")
        return sim_lib().dtwsim_cost(x_ptr, y_ptr, int(np.dtype(dtype) == np.float64), n_features, n, m, metric, c_ptr)

    def dtw_prepare_exec(self, c_ptr, dtype, count, out_ptr, work_ptr):
        SimContext.calls.append("prepare")
        return sim_lib().dtwsim_prepare(c_ptr, self.DTW_TYPES[np.dtype(dtype).name], count, out_ptr or None)

    def dtw_accumulate_exec(self, c_ptr, n, m, steps, weights_add, weights_mul, subseq, band, tile, d_ptr, idx_ptr):
        SimContext.calls.append("accumulate")
        steps = np.ascontiguousarray(steps, dtype=np.int32)
        wa, wm = np.ascontiguousarray(weights_add, dtype=np.float64), np.ascontiguousarray(weights_mul, dtype=np.float64)
        lo, hi = band if band is not None else (0, 0)
        rc = sim_lib().dtwsim_accumulate(c_ptr, n, m, steps.ctypes.data, wa.ctypes.data, wm.ctypes.data, len(steps), int(bool(subseq)), int(band is not None), lo, hi, tile, d_ptr, idx_ptr)
        assert rc > 0
        SimContext.launches.append(rc)

    def dtw_widen_exec(self, idx_ptr, count, out_ptr):
        SimContext.calls.append("widen")
        sim_lib().dtwsim_widen(idx_ptr, count, out_ptr)

    def dtw_backtrack_exec(self, d_ptr, idx_ptr, steps_i32, n, m, steps, subseq, start, path_ptr, work_ptr):
        SimContext.calls.append("backtrack")
        steps = np.ascontiguousarray(steps, dtype=np.int32)
        length = ctypes.c_longlong(0)
        status = sim_lib().dtwsim_backtrack(d_ptr or None, idx_ptr, int(bool(steps_i32)), n, m, steps.ctypes.data, len(steps), int(bool(subseq)), start, path_ptr, ctypes.addressof(length))
        assert status >= 0
        return int(length.value), status


class SimSession:
    """librosa_amd._arrays.Session with host arrays for buffers; results and scratch arrive full of 0xFF bytes: every element must be stored."""

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
        a = np.full(max(int(nbytes), 16), 0xFF, np.uint8)
        self.keep.append(a)
        return a.ctypes.data

    def close(self):
        pass


@pytest.fixture
def on_sim(monkeypatch):
    monkeypatch.setattr(S._arrays, "Session", SimSession)
    SimContext.launches, SimContext.calls = [], []
    return SimContext


class NoDevice:
    def __init__(self, like):
        raise AssertionError("the call reached the device")


# ---- the golden file and the model ---------------------------------------------------------------------------------------------------------------
def test_golden_covers_the_cases():
    arrays, meta = DC.load()
    assert set(meta["cases"]) == set(DC.CASES) and set(meta["refusals"]) == set(DC.refusals()) and set(meta["backtracks"]) == set(DC.BACKTRACKS)
    for name, c in DC.CASES.items():
        shape = meta["cases"][name]["shape"]
        transposed = c["kind"] == "XY" and c["kw"].get("subseq") and c["N"] > c["M"]
        assert shape == ([c["M"], c["N"]] if transposed else [c["N"], c["M"]]), name
        assert arrays[f"{name}/wp"].dtype == np.int64 and arrays[f"{name}/row"].shape == (shape[1],) and arrays[f"{name}/col"].shape == (shape[0],)
    # the issue's shapes: the transposed D and the flipped wp of a longer X; the flipped wp of a given C with more rows than columns
    assert meta["cases"]["xy_sub_130x70"]["shape"] == [70, 130] and arrays["xy_sub_130x70/wp"][0, 1] == 69 and arrays["xy_sub_130x70/wp"][-1, 1] == 0
    assert arrays["sub_70x33/wp"][0, 1] == 69 and arrays["sub_33x70/wp"][0, 0] == 32


@pytest.mark.parametrize("name", DC.GIVEN)
def test_model_matches_the_reference(name):
    arrays, meta = DC.load()
    a = DC.inputs(name)
    D, wp, steps = DC.model_dtw(a["C"], a["kw"])
    assert DC.sha(D) == meta["cases"][name]["sha_D"] and DC.sha(steps) == meta["cases"][name]["sha_steps"]
    assert np.array_equal(wp, arrays[f"{name}/wp"]) and np.array_equal(D[-1], arrays[f"{name}/row"]) and np.array_equal(D[:, -1], arrays[f"{name}/col"])


@pytest.mark.parametrize("name", DC.FEATURES)
def test_model_on_the_numpy_cost_is_within_delta_and_case_is_certified(name):
    arrays, meta = DC.load()
    c, a = DC.CASES[name], DC.inputs(name)
    kw = a["kw"]
    transposed = bool(kw.get("subseq")) and c["N"] > c["M"]
    C = DC.np_cost(a["X"], a["Y"], kw.get("metric", "euclidean"))
    D, wp, _ = DC.model_dtw(C.T if transposed else C, kw)
    wp = np.fliplr(wp) if transposed else wp
    entry = meta["cases"][name]
    assert entry["delta"] == DC.delta(name, D) or abs(entry["delta"] - DC.delta(name, D)) <= 1e-3 * entry["delta"]   # (ulp(max D) of the model's D, not the reference's)
    assert entry["margin"] >= DC.MARGIN_FLOOR and entry["margin"] >= DC.MARGIN_FACTOR * entry["delta"], f"{name}: margin {entry['margin']:.3g}, delta {entry['delta']:.3g}: change the seed"
    assert np.array_equal(wp, arrays[f"{name}/wp"])
    assert DC.d_error(D[-1], arrays[f"{name}/row"]) <= entry["delta"] and DC.d_error(D[:, -1], arrays[f"{name}/col"]) <= entry["delta"]


def test_band_predicate_equals_fill_off_diagonal_cells():
    # util.fill_off_diagonal's docstring examples (util/utils.py:2027-2048)
    square = ~DC.band_mask(8, 8, 0.25)
    assert square[0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0] and square[2].tolist() == [0, 1, 1, 1, 0, 0, 0, 0] and square[7].tolist() == [0, 0, 0, 0, 0, 0, 1, 1]
    wide = ~DC.band_mask(8, 12, 0.25)
    assert wide[0].tolist() == [1] * 6 + [0] * 6 and wide[7].tolist() == [0] * 6 + [1] * 6 and wide[2].tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0]


# ---- argument checks -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, r in DC.refusals().items() if not r[3]])
def test_refused_without_a_device_with_the_reference_text(name, monkeypatch):
    monkeypatch.setattr(S._arrays, "Session", NoDevice)
    fn, args, kw, _ = DC.refusals()[name]
    with pytest.raises(L.ParameterError) as e:
        getattr(S, fn)(*args, **kw)
    assert str(e.value) == DC.load()[1]["refusals"][name]


@pytest.mark.parametrize("name", [n for n, r in DC.refusals().items() if r[3]])
def test_status_words_refuse_with_the_reference_text(name, on_sim):
    fn, args, kw, _ = DC.refusals()[name]
    with pytest.raises(L.ParameterError) as e:
        getattr(S, fn)(*args, **kw)
    assert str(e.value) == DC.load()[1]["refusals"][name]
    if name.startswith("nan"):
        assert on_sim.calls == ["prepare"]   # (read before the next stage)


def test_cosine_of_a_zero_vector_is_nan_and_refused(on_sim):
    X, Y = np.ones((3, 5)), np.ones((3, 7))
    Y[:, 4] = 0.0
    with pytest.raises(L.ParameterError, match="DTW cost matrix C has NaN values"):
        S.dtw(X, Y, metric="cosine")
    assert on_sim.calls == ["cost"]


@pytest.mark.parametrize("name", list(DC.limits()))
def test_documented_differences_are_refused_before_device_work(name, monkeypatch):
    monkeypatch.setattr(S._arrays, "Session", NoDevice)
    fn, args, kw, word = DC.limits()[name]
    with pytest.raises(L.ParameterError, match=re.escape(word)):
        getattr(S, fn)(*args, **kw)


def test_limits_are_the_header_constants():
    header = open(os.path.join(ROOT, "include", "librosa_amd.h")).read()
    assert f"#define LRA_DTW_MAX_STEPS {DC.MAX_STEPS} " in header and f"#define LRA_DTW_MAX_STEP {DC.MAX_STEP} " in header
    assert (S.DTW_MAX_STEPS, S.DTW_MAX_STEP) == (DC.MAX_STEPS, DC.MAX_STEP) and S.DTW_METRICS == DC.METRICS
    kernels = open(os.path.join(ROOT, "librosa_amd", "csrc", "lra_dtw.h")).read()
    assert f"kMaxSteps = {DC.MAX_STEPS};" in kernels and f"kMaxStep = {DC.MAX_STEP};" in kernels and f"kDefaultTile = {DC.DEFAULT_TILE};" in kernels
    assert "#pragma clang fp contract(off)" in kernels


def test_exported_names():
    for name in ("dtw", "dtw_backtracking"):
        assert name in S.__all__ and callable(getattr(S, name))
    assert L.sequence.dtw is S.dtw


# ---- the kernel bodies on host fibres ----------------------------------------------------------------------------------------------------------------
def geometry(tile, max0, max1):
    out = np.zeros(6, np.int32)
    sim_lib().dtwsim_geometry(tile, max0, max1, out.ctypes.data_as(ctypes.c_void_p))
    return dict(tile=int(out[0]), d_rows=int(out[1]), d_stride=int(out[2]), off_c=int(out[3]), off_s=int(out[4]), lds=int(out[5]))


def test_launch_geometry():
    assert geometry(0, 1, 1) == dict(tile=64, d_rows=65, d_stride=66, off_c=65 * 66 * 8, off_s=65 * 66 * 8 + 64 * 64 * 8, lds=65 * 66 * 8 + 64 * 64 * 9)
    assert geometry(8, 8, 8)["d_stride"] == 16 and geometry(8, 3, 2)["d_stride"] == 10 and geometry(32, 1, 3)["d_rows"] == 33
    lib = _native.load_library()
    for tile in (0, 8, 16, 32, 64):
        for max0, max1 in ((1, 1), (3, 1), (1, 8), (8, 8)):
            g = geometry(tile, max0, max1)
            assert g["lds"] <= 160 * 1024 and g["d_stride"] % 2 == 0 and g["d_stride"] >= g["tile"] + max1 and g["off_c"] % 8 == 0
            assert g["lds"] == lib.lra_dtw_lds_bytes(tile, max0, max1)
    assert lib.lra_dtw_lds_bytes(24, 1, 1) == 0 and lib.lra_dtw_lds_bytes(64, 9, 1) == 0


worst = {}


@pytest.mark.parametrize("name", list(DC.CASES))
def test_kernel_bodies_on_the_host(name, on_sim):
    c = DC.CASES[name]
    D, wp, steps = DC.run_case(name, S)
    worst[name] = DC.check_case(name, np.asarray(D), np.asarray(wp), np.asarray(steps), report=print)
    tile = c["tile"] or DC.DEFAULT_TILE
    assert on_sim.launches == [-(-D.shape[0] // tile) + -(-D.shape[1] // tile) - 1]   # one launch per tile anti-diagonal
    assert on_sim.calls == ["prepare" if c["kind"] == "C" else "cost", "accumulate", "backtrack", "widen"]


@pytest.mark.parametrize("name", ["t8_20x37", "t8_37x20", "t16_65x70", "t32_65x70", "s313_t8_66x90", "s8_t8_40x47", "gc_t8_40x50"])
def test_forced_tile_equals_the_default_tile_on_the_host(name, on_sim):
    forced = DC.run_case(name, S)
    default = DC.run_case(name, S, tile=0)
    assert on_sim.launches[0] > on_sim.launches[1]
    for a, b in zip(forced, default):
        assert np.array_equal(a, b)


def test_return_combinations_on_the_host(on_sim):
    a = DC.inputs("c_63x65_rand")
    D, wp, steps = S.dtw(C=a["C"], return_steps=True)
    on_sim.calls.clear()
    only = S.dtw(C=a["C"], backtrack=False)
    assert isinstance(only, np.ndarray) and np.array_equal(only, D) and on_sim.calls == ["prepare", "accumulate"]
    D2, wp2 = S.dtw(C=a["C"])
    assert np.array_equal(D2, D) and np.array_equal(wp2, wp)
    D3, steps3 = S.dtw(C=a["C"], backtrack=False, return_steps=True)
    assert np.array_equal(D3, D) and np.array_equal(steps3, steps) and steps3.dtype == np.int32


@pytest.mark.parametrize("name", list(DC.BACKTRACKS))
def test_dtw_backtracking_on_the_host(name, on_sim):
    case, kw = DC.BACKTRACKS[name]
    a = DC.inputs(case)
    steps = DC.model(a["C"], a["kw"])[1]
    before = steps.copy()
    wp = S.dtw_backtracking(steps, **kw)
    assert wp.dtype == np.int64 and np.array_equal(wp, DC.load()[0][f"{name}/wp"]) and np.array_equal(steps, before)
    assert on_sim.calls == ["backtrack"]
    wp8 = S.dtw_backtracking(steps.astype(np.uint8), **kw)   # (any integer type of steps)
    assert np.array_equal(wp8, wp)


def test_dtw_backtracking_stops_where_an_index_goes_negative(on_sim):
    # step 0 = (1, 1) everywhere: from (3, 1) the walk reaches (2, 0) and would leave the matrix; the reference breaks there (:634)
    steps = np.zeros((4, 2), dtype=np.int32)
    assert S.dtw_backtracking(steps).tolist() == [[3, 1], [2, 0]]
    assert S.dtw_backtracking(steps, subseq=True, start=0).tolist() == [[3, 0]]


def test_dtw_backtracking_refuses_an_index_outside_the_step_table(on_sim):
    steps = np.zeros((6, 9), dtype=np.int32)
    steps[4, 7] = 3
    with pytest.raises(L.ParameterError, match="outside the step table"):
        S.dtw_backtracking(steps)
    assert len(S.dtw_backtracking(steps, step_sizes_sigma=[[2, 1]])) > 1
    steps[4, 7] = -1
    with pytest.raises(L.ParameterError, match="outside the step table"):
        S.dtw_backtracking(steps)
