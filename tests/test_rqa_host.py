"""sequence.rqa without a GPU: the golden file against the cases, the NumPy model against the golden, the argument checks that need no device,
the documented differences, the exported names, and the kernel bodies of librosa_amd/csrc/lra_rqa.h run on host fibres
(tests/hostsim/rqasim.cpp) behind the package's own Python layer (a session whose buffers are host arrays, results full of 0xFF bytes).

Through the simulator every case is bit-equal in ``score`` and equal in ``path``, and the pointers equal the model's."""
import ctypes
import os
import re

import numpy as np
import pytest

import hostsim_util
import librosa_amd as L
import rqa_cases as RC
from librosa_amd import _native
from librosa_amd import sequence as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_sim = None


def sim_lib():
    global _sim
    if _sim is None:
        _sim = hostsim_util.sim_lib("rqasim", pthread=False)
        c = ctypes
        _sim.rqasim_geometry.argtypes = [c.c_int, c.c_int, c.c_void_p]
        _sim.rqasim_served.argtypes = [c.c_int, c.c_int]
        _sim.rqasim_prepare.argtypes = [c.c_void_p, c.c_int, c.c_longlong, c.c_void_p]
        _sim.rqasim_score.argtypes = [c.c_void_p, c.c_int, c.c_longlong, c.c_longlong, c.c_double, c.c_double, c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_void_p]
        _sim.rqasim_score.restype = c.c_longlong
        _sim.rqasim_argmax.argtypes = [c.c_void_p, c.c_int, c.c_longlong, c.c_void_p]
        _sim.rqasim_backtrack.argtypes = [c.c_void_p, c.c_longlong, c.c_longlong, c.c_void_p, c.c_void_p]
        _sim.rqasim_backtrack.restype = c.c_longlong
    return _sim


class SimContext:
    """The native calls of librosa_amd.sequence's RQA, served by the simulator on host pointers."""

    DTW_TYPES, RQA_WORK_BYTES = _native.Context.DTW_TYPES, _native.Context.RQA_WORK_BYTES
    launches = []   # per scoring call: the number of kernel launches
    calls = []      # the native calls made, by name
    pointers = []   # per scoring call: (address, n, m) of the pointers

    def dtw_prepare_exec(self, c_ptr, dtype, count, out_ptr, work_ptr):
        SimContext.calls.append("prepare")
        return sim_lib().rqasim_prepare(c_ptr, self.DTW_TYPES[np.dtype(dtype).name], count, out_ptr or None)

    def rqa_score_exec(self, sim_ptr, dtype, n, m, gap_onset, gap_extend, knight_moves, rows, strip, score_ptr, pointers_ptr):
        SimContext.calls.append("score")
        rc = sim_lib().rqasim_score(sim_ptr, int(np.dtype(dtype) == np.float64), n, m, float(gap_onset), float(gap_extend), int(bool(knight_moves)), rows, strip, score_ptr, pointers_ptr)
        assert rc > 0
        SimContext.launches.append(rc)
        SimContext.pointers.append((pointers_ptr, n, m))

    def rqa_argmax_exec(self, score_ptr, dtype, count, work_ptr):
        SimContext.calls.append("argmax")
        sim_lib().rqasim_argmax(score_ptr, int(np.dtype(dtype) == np.float64), count, work_ptr)

    def rqa_backtrack_exec(self, pointers_ptr, n, m, work_ptr, path_ptr):
        SimContext.calls.append("backtrack")
        return int(sim_lib().rqasim_backtrack(pointers_ptr, n, m, work_ptr, path_ptr))


class SimSession:
    """librosa_amd._arrays.Session with host arrays for buffers; results and scratch arrive full of 0xFF bytes: every element must be stored."""

    is_torch = False
    last = None

    def __init__(self, like):
        self.ctx, self.keep = SimContext(), []
        SimSession.last = self

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
    SimContext.launches, SimContext.calls, SimContext.pointers = [], [], []
    return SimContext


def last_pointers():
    """The pointers of the last scoring call, out of the session's scratch."""
    address, n, m = SimContext.pointers[-1]
    return np.ctypeslib.as_array((ctypes.c_int8 * (n * m)).from_address(address)).reshape(n, m).copy()


class NoDevice:
    def __init__(self, like):
        raise AssertionError("the call reached the device")


# ---- the golden file and the model ---------------------------------------------------------------------------------------------------------------
def test_golden_covers_the_cases():
    arrays, meta = RC.load()
    assert set(meta["cases"]) == set(RC.CASES) and set(meta["refusals"]) == set(RC.refusals())
    for name, c in RC.CASES.items():
        entry = meta["cases"][name]
        assert entry["shape"] == [c["N"], c["M"]], name
        assert arrays[f"{name}/path"].dtype == np.uint64 and arrays[f"{name}/path"].shape[1:] == (2,)
        assert arrays[f"{name}/row"].shape == (c["M"],) and arrays[f"{name}/col"].shape == (c["N"],) and arrays[f"{name}/row"].dtype == RC.expected_dtype(name)
        assert entry["left"] == (name in RC.QUIRKS), f"{name}: only the quirk cases may leave the matrix; change its seed"
    assert meta["tie_case"] in RC.CASES and RC.CASES[meta["tie_case"]]["kind"] == "binary"
    # what the issue lists: every init shape, forced geometry and gap setting with knight moves on and off, every kind of input, every type
    for N, M in RC.INIT_SHAPES:
        assert any((c["N"], c["M"]) == (N, M) for c in RC.CASES.values())
    for rows, strip, N, M in RC.FORCED + RC.SHIPPED:
        for gaps in RC.GAPS:
            for knight in (True, False):
                assert any((c["rows"], c["strip"], c["N"], c["M"], c["gaps"], c["knight"]) == (rows, strip, N, M, gaps, knight) for c in RC.CASES.values())
        for kind in RC.KINDS:
            assert any((c["rows"], c["strip"], c["N"], c["M"], c["kind"]) == (rows, strip, N, M, kind) for c in RC.CASES.values())
    assert {c["dtype"] for c in RC.CASES.values()} >= {"float32", "float64", "bool", "uint8", "int32", "int64"}
    assert arrays[f"{RC.QUIRKS[0]}/path"].tolist() == [[2, 1], [3, 2], [4, 3]]                 # the reference's walk, cut short
    assert arrays[f"{RC.QUIRKS[1]}/path"].tolist()[0] == [1, 2**64 - 1]                         # and through column -1


def test_shipped_shapes_straddle_the_shipped_constants():
    kernels = open(os.path.join(ROOT, "librosa_amd", "csrc", "lra_rqa.h")).read()
    assert f"kDefaultRows = {RC.DEFAULT_ROWS};" in kernels and f"kDefaultStrip = {RC.DEFAULT_STRIP};" in kernels
    assert "#pragma clang fp contract(off)" in kernels
    g = geometry(0, 0)
    assert (g["rows"], g["strip"]) == (RC.DEFAULT_ROWS, RC.DEFAULT_STRIP)
    (_, _, n1, m1), (_, _, n2, m2) = RC.SHIPPED
    assert g["rows"] < n1 <= 2 * g["rows"] and g["strip"] < m1 <= 2 * g["strip"]        # two launches, two strips, the second of each nearly empty
    assert 2 * g["rows"] < n2 <= 3 * g["rows"] and 2 * g["strip"] < m2 <= 3 * g["strip"]  # three of each


@pytest.mark.parametrize("name", list(RC.CASES))
def test_model_matches_the_reference(name):
    arrays, meta = RC.load()
    entry = meta["cases"][name]
    sim = RC.inputs(name)
    score, path, ptr = RC.model_rqa(sim, **RC.kwargs(name))
    assert score.dtype == RC.expected_dtype(name) and RC.sha(score) == entry["sha_score"]
    assert np.array_equal(score[-1], arrays[f"{name}/row"], equal_nan=True) and np.array_equal(score[:, -1], arrays[f"{name}/col"], equal_nan=True)
    as_reference, left = RC.walk(score, ptr, reference=True)
    assert left == entry["left"] and np.array_equal(as_reference, arrays[f"{name}/path"])   # (the reference's reading, its quirk included)
    if not left:
        assert np.array_equal(path, arrays[f"{name}/path"])


def test_quirk_paths_follow_the_moves_that_were_scored():
    for name in RC.QUIRKS:
        path = RC.model_rqa(RC.inputs(name), **RC.kwargs(name))[1]
        assert path.tolist() == [[0, 0], [2, 1], [3, 2], [4, 3]]


# ---- argument checks -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.refusals()))
def test_refused_without_a_device_with_the_reference_text(name, monkeypatch):
    monkeypatch.setattr(S._arrays, "Session", NoDevice)
    with pytest.raises(L.ParameterError) as e:
        S.rqa(np.ones((4, 5)), **RC.refusals()[name])
    assert str(e.value) == RC.load()[1]["refusals"][name]
    with pytest.raises(L.ParameterError) as e:   # (the gaps are checked before sim, as in the reference)
        S.rqa(np.ones(5), **RC.refusals()[name])
    assert str(e.value) == RC.load()[1]["refusals"][name]


def test_refusal_texts_keep_their_braces():
    texts = RC.load()[1]["refusals"]
    assert texts["gap_onset"] == "gap_onset={} must be strictly positive" and texts["gap_extend"] == "gap_extend={} must be strictly positive"
    assert texts["both"] == texts["gap_onset"]


@pytest.mark.parametrize("name", list(RC.limits()))
def test_documented_differences_are_refused_before_device_work(name, monkeypatch):
    monkeypatch.setattr(S._arrays, "Session", NoDevice)
    sim, word = RC.limits()[name]
    with pytest.raises(L.ParameterError, match=re.escape(word)):
        S.rqa(sim)


def test_exported_names():
    assert "rqa" in S.__all__ and callable(S.rqa) and L.sequence.rqa is S.rqa
    assert (S.RQA_ROWS, S.RQA_STRIP) == (0, 0)
    assert "rqa" in S.__doc__ and "4.6p" in S.__doc__
    header = open(os.path.join(ROOT, "include", "librosa_amd.h")).read()
    assert f"#define LRA_RQA_WORK_BYTES ({_native.Context.RQA_WORK_BYTES - 16 * 1024} + 16 * 1024)" in header
    for name in ("lra_rqa_lds_bytes", "lra_rqa_score_exec", "lra_rqa_argmax_exec", "lra_rqa_backtrack_exec"):
        assert name in _native.SIGNATURES and name in header
    import librosa_amd._arrays as A

    assert A.torch_dtype(np.uint64) is __import__("torch").uint64


# ---- the kernel bodies on host fibres ----------------------------------------------------------------------------------------------------------------
def geometry(rows, strip):
    out = np.zeros(7, np.int32)
    sim_lib().rqasim_geometry(rows, strip, out.ctypes.data_as(ctypes.c_void_p))
    return dict(zip(("rows", "strip", "halo", "width", "nt", "iters", "lds"), (int(v) for v in out)))


def test_launch_geometry():
    assert geometry(16, 16) == dict(rows=16, strip=16, halo=30, width=48, nt=64, iters=1, lds=3 * 48 * 16)
    assert geometry(64, 1024)["iters"] == 5 and geometry(64, 1024)["lds"] <= 64 * 1024 and geometry(1, 4)["halo"] == 0
    assert (geometry(32, 128)["nt"], geometry(32, 128)["iters"]) == (192, 1) and (geometry(64, 256)["nt"], geometry(64, 256)["iters"]) == (256, 2)
    lib = _native.load_library()
    for rows in (0, 1, 2, 3, 4, 8, 16, 24, 32, 64, 128, -1):
        for strip in (0, 2, 4, 8, 16, 48, 256, 512, 1024, 2048, -4):
            if sim_lib().rqasim_served(rows, strip):
                g = geometry(rows, strip)
                assert lib.lra_rqa_lds_bytes(rows, strip) == g["lds"] > 0 and g["lds"] % 16 == 0 and g["width"] == g["strip"] + 2 * (g["rows"] - 1) + 2
                assert g["iters"] * g["nt"] >= g["strip"] + g["halo"] and 1 <= g["iters"] <= 5 and g["nt"] % 64 == 0 and 64 <= g["nt"] <= 256
            else:
                assert lib.lra_rqa_lds_bytes(rows, strip) == 0
    assert sim_lib().rqasim_served(0, 0) and sim_lib().rqasim_served(64, 1024) and not sim_lib().rqasim_served(3, 4) and not sim_lib().rqasim_served(4, 2048)


@pytest.mark.parametrize("name", list(RC.CASES))
def test_kernel_bodies_on_the_host(name, on_sim):
    c = RC.CASES[name]
    score, path = RC.run_case(name, S)
    assert isinstance(score, np.ndarray) and isinstance(path, np.ndarray)
    RC.check_case(name, score, path)
    assert np.array_equal(last_pointers(), RC.model(RC.inputs(name), **RC.kwargs(name))[1])
    rows, strip = RC.geometry(name)
    assert on_sim.launches == [-(-c["N"] // rows)]   # one launch per block of rows
    assert on_sim.calls == (["prepare"] if c["dtype"] in ("bool", "uint8", "int32", "int64") else []) + ["score", "argmax", "backtrack"]


@pytest.mark.parametrize("name", [n for n, c in RC.CASES.items() if c["rows"] and c["kind"] in ("binary", "sparse") and c["dtype"] == "float64"])
def test_forced_geometry_equals_the_default_geometry_on_the_host(name, on_sim):
    forced = RC.run_case(name, S)
    default = RC.run_case(name, S, geometry=(0, 0))
    assert on_sim.launches[0] > on_sim.launches[1] == -(-forced[0].shape[0] // RC.DEFAULT_ROWS)
    for a, b in zip(forced, default):
        assert np.array_equal(a, b, equal_nan=True)


def test_backtrack_false_and_the_empty_path_on_the_host(on_sim):
    sim = RC.inputs(next(n for n, c in RC.CASES.items() if c["kind"] == "sparse" and (c["N"], c["M"]) == (20, 37)))
    only = S.rqa(sim, backtrack=False)
    assert isinstance(only, np.ndarray) and on_sim.calls == ["score"]
    score, path = S.rqa(sim)
    assert np.array_equal(only, score) and len(path) > 0
    score, path = S.rqa(np.zeros((5, 9), dtype=np.float32))
    assert path.shape == (0, 2) and path.dtype == np.uint64 and score.dtype == np.float32 and not score.any()


def test_argmax_takes_the_first_maximum_and_a_nan_first_on_the_host():
    work = np.full(_native.Context.RQA_WORK_BYTES, 0xFF, np.uint8)
    rng = np.random.default_rng(31)
    for count in (1, 255, 4096, 4097, 70000):
        for dtype in (np.float32, np.float64):
            a = rng.integers(0, 5, size=count).astype(dtype)   # (ties everywhere)
            sim_lib().rqasim_argmax(a.ctypes.data, int(dtype == np.float64), count, work.ctypes.data)
            assert int(work[:8].view(np.int64)[0]) == int(np.argmax(a))
            a[[count // 2, count - 1]] = np.nan
            sim_lib().rqasim_argmax(a.ctypes.data, int(dtype == np.float64), count, work.ctypes.data)
            assert int(work[:8].view(np.int64)[0]) == int(np.argmax(a)) == count // 2
