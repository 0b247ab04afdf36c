"""segment.recurrence_matrix and cross_similarity without a GPU: the golden file against the cases, the NumPy model against the golden, the
argument checks that need no device, the exported names, and the kernel bodies of librosa_amd/csrc/lra_knn.h run on host fibres
(tests/hostsim/knnsim.cpp) behind the package's own Python layer (a session whose buffers are host arrays, results full of 0xFF bytes).

Through the simulator every case meets the rule of judgement of tests/knn_cases.py against the golden and is bit-equal to the model (an affinity
within the two units in the last place that separate two exp implementations); the tie cases, which the reference cannot judge, are bit-equal to
the model at every forced geometry."""
import ctypes
import os

import numpy as np
import pytest

import hostsim_util
import knn_cases as KC
import librosa_amd as L
from librosa_amd import _native
from librosa_amd import segment as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_sim = None


def sim_lib():
    global _sim
    if _sim is None:
        _sim = hostsim_util.sim_lib("knnsim", pthread=False)
        c = ctypes
        p, i, q, d = c.c_void_p, c.c_int, c.c_longlong, c.c_double
        _sim.knnsim_lds_bytes.argtypes = [i, i, i]
        _sim.knnsim_lds_bytes.restype = q
        _sim.knnsim_geometry.argtypes = [i, i, i, q, p]
        _sim.knnsim_select.argtypes = [p, p, i, q, q, q, i, i, q, i, i, i, p, p, p]
        _sim.knnsim_mutual.argtypes = [q, i, p, p, p, i, i, p]
        _sim.knnsim_bandwidth.argtypes = [q, i, p, p, p, i, i, i, p, p, p]
        _sim.knnsim_bw_check.argtypes = [p, q]
        _sim.knnsim_emit.argtypes = [q, q, i, p, p, p, p, i, i, i, d, i, p, p, p, p, p, p, p, p]
        _sim.knnsim_emit.restype = q
        _sim.knnsim_dense.argtypes = [p, p, i, q, q, q, i, q, i, i, i, d, i, p, p, p, p]
    return _sim


class SimContext:
    """The native calls of librosa_amd.segment, served by the simulator on host pointers."""

    C = _native.Context
    DTW_METRICS, KNN_MODES, KNN_BW_MODES, KNN_WORK_BYTES = C.DTW_METRICS, C.KNN_MODES, C.KNN_BW_MODES, C.KNN_WORK_BYTES
    KNN_BW_SCALAR, KNN_BW_MATRIX = C.KNN_BW_SCALAR, C.KNN_BW_MATRIX
    KNN_STATUS_EMPTY_GRAPH, KNN_STATUS_ROW_EMPTY, KNN_STATUS_NON_POSITIVE = C.KNN_STATUS_EMPTY_GRAPH, C.KNN_STATUS_ROW_EMPTY, C.KNN_STATUS_NON_POSITIVE
    calls = []      # the native calls made, by name
    selects = []    # per selection: (rows, tile, k, n)

    def knn_select_exec(self, q_ptr, r_ptr, dtype, n_features, n, m, metric, k, width, skip_zero, rows, tile, count_ptr, index_ptr, distance_ptr):
        SimContext.calls.append("select")
        SimContext.selects.append((rows, tile, k, n))
        assert sim_lib().knnsim_select(q_ptr, r_ptr, int(np.dtype(dtype) == np.float64), n_features, n, m, metric, k, width, int(skip_zero), rows, tile, count_ptr, index_ptr, distance_ptr) == 0

    def knn_mutual_exec(self, n, k, count_ptr, index_ptr, distance_ptr, sym, drop_zero, keep_ptr):
        SimContext.calls.append("mutual")
        sim_lib().knnsim_mutual(n, k, count_ptr, index_ptr, distance_ptr, int(bool(sym)), int(bool(drop_zero)), keep_ptr)

    def knn_bandwidth_exec(self, n, k, count_ptr, distance_ptr, keep_ptr, add_self, bandwidth_k, median, dist_to_k_ptr, avg_ptr, work_ptr):
        SimContext.calls.append("bandwidth")
        sim_lib().knnsim_bandwidth(n, k, count_ptr, distance_ptr, keep_ptr or None, int(bool(add_self)), bandwidth_k, int(bool(median)), dist_to_k_ptr, avg_ptr, work_ptr)
        status = np.ctypeslib.as_array((ctypes.c_int32 * 2).from_address(work_ptr))
        return int(status[0]), int(status[1])

    def knn_bw_check_exec(self, matrix_ptr, count, work_ptr):
        SimContext.calls.append("bw_check")
        return int(sim_lib().knnsim_bw_check(matrix_ptr, count))

    def knn_emit_exec(self, n, m, k, count_ptr, index_ptr, distance_ptr, keep_ptr, self_link, mode, bw_mode, bw_scalar, bw_on_device, sigma_ptr, matrix_ptr, work_ptr, counts_ptr, indptr_ptr,
                      indices_ptr, data_ptr, dense_ptr):
        SimContext.calls.append("emit")
        return int(sim_lib().knnsim_emit(n, m, k, count_ptr, index_ptr, distance_ptr, keep_ptr, int(bool(self_link)), mode, bw_mode, float(bw_scalar), int(bool(bw_on_device)), sigma_ptr or None,
                                         matrix_ptr or None, work_ptr, counts_ptr or None, indptr_ptr or None, indices_ptr or None, data_ptr or None, dense_ptr or None))

    def knn_dense_exec(self, q_ptr, r_ptr, dtype, n_features, n, m, metric, width, self_link, mode, bw_mode, bw_scalar, bw_on_device, sigma_ptr, matrix_ptr, work_ptr, out_ptr):
        SimContext.calls.append("dense")
        sim_lib().knnsim_dense(q_ptr, r_ptr, int(np.dtype(dtype) == np.float64), n_features, n, m, metric, width, int(bool(self_link)), mode, bw_mode, float(bw_scalar), int(bool(bw_on_device)),
                               sigma_ptr or None, matrix_ptr or None, work_ptr, out_ptr)


class SimSession:
    """librosa_amd._arrays.Session with host arrays for buffers; results and scratch arrive full of 0xFF bytes: every element must be stored."""

    is_torch = False
    scratch_bytes = 0

    def __init__(self, like):
        self.ctx, self.keep = SimContext(), []
        SimSession.scratch_bytes = 0

    def input_raw(self, a, dtype):
        a = np.array(a, dtype=dtype, copy=True, order="C")
        self.keep.append(a)
        return a.ctypes.data

    def output(self, shape, dtype, rows=False):
        a = np.frombuffer(bytearray(b"\xff" * max(16, int(np.prod(shape)) * np.dtype(dtype).itemsize)), dtype=dtype)[: int(np.prod(shape))].reshape(shape)
        self.keep.append(a)
        SimSession.scratch_bytes += a.nbytes
        return a.ctypes.data, a

    def result(self, handle):
        return handle

    def scratch(self, nbytes):
        a = np.full(max(int(nbytes), 16), 0xFF, np.uint8)
        self.keep.append(a)
        SimSession.scratch_bytes += a.nbytes
        return a.ctypes.data

    def close(self):
        pass


@pytest.fixture
def on_sim(monkeypatch):
    monkeypatch.setattr(G._arrays, "Session", SimSession)
    SimContext.calls, SimContext.selects = [], []
    return SimContext


class NoDevice:
    def __init__(self, like):
        raise AssertionError("the call reached the device")


# ---- the golden file and the model ---------------------------------------------------------------------------------------------------------------
def test_golden_covers_the_cases():
    arrays, meta = KC.load()
    assert set(meta["cases"]) == set(KC.CASES) and set(meta["refusals"]) == set(KC.refusals())
    for name, c in KC.CASES.items():
        entry = meta["cases"][name]
        if "refused" in entry:
            continue
        n_ref = c["n"] if c["fn"] == "rec" else c["n_ref"]
        assert entry["shape"] == [n_ref, c["n"]] and arrays[f"{name}/result"].shape == (n_ref, c["n"]), name
        rel, ab = KC.value_tolerance(name)
        assert entry["margin"] is None or entry["margin"] > 1000 * max(rel, ab), f"{name}: the selection margin is within 1000 tolerances; change its seed"
    # what the issue lists
    rec = [c for c in KC.CASES.values() if c["fn"] == "rec"]
    cross = [c for c in KC.CASES.values() if c["fn"] == "cross"]
    assert {c["n"] for c in rec} >= {5, 7, 9, 33, 70, KC.DEFAULT_TILE + 3, 2 * KC.DEFAULT_TILE + 3}
    assert {(c["n"], c["kw"]["width"]) for c in rec} >= {(5, 1), (7, 2), (9, 3)}
    assert {(c["n_ref"], c["n"]) for c in cross} >= {(1, 1), (1, 7), (7, 1), (5, 9), (9, 5), (33, 70), (70, 33)}
    assert {c["d"] for c in KC.CASES.values()} >= {1, 3, 12, 40} and {c["metric"] for c in KC.CASES.values()} == set(KC.METRICS)
    for mode in KC.MODES:
        for sym in (False, True):
            for self_link in (False, True):
                assert any((c["kw"]["mode"], c["kw"]["sym"], c["kw"]["self"]) == (mode, sym, self_link) for c in rec if "self" in c["kw"] and "sym" in c["kw"])
    for full in (False, True):
        for bw in (None, 0.7, "matrix", *KC.BW_MODES[1:]):
            for cases in (rec, cross):
                assert any(c["kw"].get("full", False) == full and c["kw"].get("bandwidth", 0) == bw and c["kw"]["mode"] == "affinity" for c in cases), (full, bw)
    assert {c["geometry"] for c in KC.CASES.values()} == {(0, 0), (1, 4), (4, 8), (8, 16)}
    for rows, tile in ((1, 4), (4, 8), (8, 16)):
        assert {c["kw"]["k"] for c in KC.CASES.values() if c["geometry"] == (rows, tile)} == {tile - 1, tile, tile + 1}
    assert {c["dtype"] for c in KC.CASES.values()} >= {"float32", "float64", "int32", "int16"} and {c["layout"] for c in KC.CASES.values()} == {"plain", "lead23", "axis0", "axis1"}
    assert any(c["kw"].get("sparse") for c in KC.CASES.values()) and any(not c["kw"].get("sparse") for c in KC.CASES.values())
    # the documented difference: the reference's connectivity pattern is not its own distance pattern for recurrence_matrix, and is for cross_similarity
    differs = meta["connectivity_differs_from_distance"]
    assert differs["rec"][0] > 0 and differs["cross"][0] == 0


def test_shipped_shapes_straddle_the_shipped_constants():
    kernels = open(os.path.join(ROOT, "librosa_amd", "csrc", "lra_knn.h")).read()
    assert f"kDefaultRows = {KC.DEFAULT_ROWS}, kDefaultTile = {KC.DEFAULT_TILE};" in kernels and f"kMaxK = {KC.MAX_K};" in kernels
    assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "librosa_amd", "csrc", "lra_dtw.h")).read()
    assert G.KNN_MAX_K == KC.MAX_K == _native.Context.KNN_MAX_K


@pytest.mark.parametrize("name", list(KC.CASES))
def test_model_matches_the_reference(name):
    entry = KC.load()[1]["cases"][name]
    if "refused" in entry:   # (a per-point bandwidth and a frame without a neighbour: the model's first empty row is the one the reference names)
        empty = np.flatnonzero((KC.model(name)[0] == 0).all(axis=0))
        assert entry["refused"] == f"The sample at time point {empty[0]} has no neighbors"
        return
    KC.check_case(name, KC.model(name)[0])


def test_duplicates_pin_the_zero_distance_rule():
    arrays, _ = KC.load()
    rec, cross, _ = KC.DUPLICATES
    # recurrence_matrix looks at non-zero links only: every frame keeps its k = 3; cross_similarity takes its 3 neighbours and then drops the zeros
    assert ((arrays[f"{rec}/result"] != 0).sum(axis=0) == 3).all()
    kept = (arrays[f"{cross}/result"] != 0).sum(axis=0)
    assert kept.max() == 2 and sorted(np.flatnonzero(kept == 1)) == [5, 12, 25, 30]   # (the frame itself is at distance 0; the four with a duplicate lose two links)


# ---- argument checks -------------------------------------------------------------------------------------------------------------------------------
DEVICE_REFUSALS = ("bw_matrix_sign", "no_neighbors", "empty_graph")   # raised from status words the kernels leave


@pytest.mark.parametrize("name", [n for n in KC.refusals() if n not in DEVICE_REFUSALS])
def test_refused_without_a_device_with_the_reference_text(name, monkeypatch):
    monkeypatch.setattr(G._arrays, "Session", NoDevice)
    with pytest.raises(L.ParameterError) as e:
        KC.refusal_call(G, name)
    assert str(e.value) == KC.load()[1]["refusals"][name]


@pytest.mark.parametrize("name", DEVICE_REFUSALS)
def test_refused_from_the_status_words_with_the_reference_text(name, on_sim):
    with pytest.raises(L.ParameterError) as e:
        KC.refusal_call(G, name)
    assert str(e.value) == KC.load()[1]["refusals"][name]


def test_documented_differences_are_refused_before_device_work(monkeypatch):
    monkeypatch.setattr(G._arrays, "Session", NoDevice)
    x = np.random.default_rng(5).standard_normal((3, 9))
    with pytest.raises(L.ParameterError, match="euclidean, sqeuclidean, cityblock, manhattan, cosine"):
        G.recurrence_matrix(x, metric="chebyshev")
    with pytest.raises(L.ParameterError, match="euclidean, sqeuclidean"):
        G.cross_similarity(x, x, metric=lambda a, b: 0.0)
    with pytest.raises(L.ParameterError, match="real-valued"):
        G.recurrence_matrix(x.astype(np.complex128))
    with pytest.raises(L.ParameterError, match="empty"):
        G.cross_similarity(np.zeros((3, 0)), x)
    with pytest.raises(L.ParameterError, match="empty"):
        G.recurrence_matrix(np.zeros((0, 9)))
    with pytest.raises(L.ParameterError, match="positive integer"):
        G.recurrence_matrix(x, k=0)
    big = np.zeros((1, 3 * KC.MAX_K))
    with pytest.raises(L.ParameterError, match=f"KNN_MAX_K={KC.MAX_K}"):
        G.recurrence_matrix(big, k=KC.MAX_K + 1)
    with pytest.raises(L.ParameterError, match=f"KNN_MAX_K={KC.MAX_K}"):
        G.cross_similarity(big, big, k=KC.MAX_K + 1)
    with pytest.raises(L.ParameterError, match=f"KNN_MAX_K={KC.MAX_K}"):
        G.recurrence_matrix(big, k=KC.MAX_K + 1, mode="affinity", full=True)
    with pytest.raises(L.ParameterError, match="n_ref=9"):
        G.cross_similarity(x[:, :5], x, mode="affinity", bandwidth="mean_k")


def test_exported_names():
    assert "segment" in L.__all__ and L.segment is G and G.__all__ == ["cross_similarity", "recurrence_matrix"]
    assert (G.KNN_ROWS, G.KNN_TILE) == (0, 0) and "4.6q" in G.__doc__ and "segment.cross_similarity" in L.__doc__
    from librosa_amd import build

    assert "knn_inst" in build.UNITS
    header = open(os.path.join(ROOT, "include", "librosa_amd.h")).read()
    assert f"#define LRA_KNN_MAX_K {_native.Context.KNN_MAX_K}" in header and f"#define LRA_KNN_WORK_BYTES {_native.Context.KNN_WORK_BYTES}" in header
    api = open(os.path.join(ROOT, "librosa_amd", "csrc", "lra_knn_inst.hip")).read()  # the unit that defines the entry points, beside their kernels
    for name in ("lra_knn_lds_bytes", "lra_knn_select_exec", "lra_knn_mutual_exec", "lra_knn_bandwidth_exec", "lra_knn_bw_check_exec", "lra_knn_emit_exec", "lra_knn_dense_exec"):
        assert name in _native.SIGNATURES and name in header and name in api
    for word, code in list(_native.Context.KNN_MODES.items()) + [("bw_" + k, v) for k, v in _native.Context.KNN_BW_MODES.items() if v]:
        assert f"#define LRA_KNN_{word.upper()} {code}" in header


def test_signatures_are_the_reference_s():
    import inspect

    rec, cross = inspect.signature(G.recurrence_matrix), inspect.signature(G.cross_similarity)
    assert str(rec) == "(data, *, k=None, width=1, metric='euclidean', sym=False, sparse=False, mode='connectivity', bandwidth=None, self=False, axis=-1, full=False)"
    assert str(cross) == "(data, data_ref, *, k=None, metric='euclidean', sparse=False, mode='connectivity', bandwidth=None, full=False)"


# ---- the kernel bodies on host fibres ----------------------------------------------------------------------------------------------------------------
def geometry(rows, tile, k, n=1):
    out = np.zeros(4, np.int64)
    sim_lib().knnsim_geometry(rows, tile, k, n, out.ctypes.data_as(ctypes.c_void_p))
    return dict(zip(("rows", "tile", "lds", "workgroups"), (int(v) for v in out)))


def test_launch_geometry():
    lib = _native.load_library()
    assert geometry(0, 0, 72)["rows"] == KC.DEFAULT_ROWS and geometry(0, 0, 72)["tile"] == KC.DEFAULT_TILE
    assert geometry(0, 0, 1024)["lds"] > 0 and geometry(0, 0, KC.MAX_K)["lds"] > 0 and geometry(0, 0, KC.MAX_K)["rows"] < KC.DEFAULT_ROWS   # fewer rows where the lists are long
    assert geometry(0, 0, KC.MAX_K + 1)["lds"] == 0 and geometry(0, 0, 0)["lds"] == 0
    for rows in (0, 1, 2, 3, 4, 8, 16, 32, -1):
        for tile in (0, 2, 4, 8, 16, 48, 128, 256, 1024, 2048):
            for k in (1, 7, 72, 228, 1024, KC.MAX_K):
                g = geometry(rows, tile, k)
                assert lib.lra_knn_lds_bytes(rows, tile, k) == g["lds"] == sim_lib().knnsim_lds_bytes(rows, tile, k)
                if g["lds"]:
                    assert g["lds"] <= 64 * 1024 and g["rows"] * g["tile"] <= 2048 and (rows in (0, g["rows"])) and (tile in (0, g["tile"]))
                    assert g["lds"] >= 12 * g["rows"] * k + 8 * g["rows"] * g["tile"]
    assert geometry(3, 8, 4)["lds"] == 0 and geometry(32, 8, 4)["lds"] == 0 and geometry(4, 48, 4)["lds"] == 0 and geometry(16, 256, 4)["lds"] == 0
    assert geometry(16, 128, KC.MAX_K)["lds"] == 0   # (the forced rows do not fit; the library's choice takes fewer)


HOST_CASES = [n for n, c in KC.CASES.items() if c["n"] <= 70 and (c["n_ref"] <= 70)] + [n for n, c in KC.CASES.items() if c["n"] == KC.DEFAULT_TILE + 3 and c["kw"]["mode"] == "distance"]


@pytest.mark.parametrize("name", HOST_CASES)
def test_kernel_bodies_on_the_host(name, on_sim):
    entry = KC.load()[1]["cases"][name]
    if "refused" in entry:
        with pytest.raises(L.ParameterError) as e:
            KC.call(G, name)
        assert str(e.value) == entry["refused"]
        return
    c = KC.CASES[name]
    result = KC.call(G, name)
    assert (type(result).__name__ == "csc_array") == bool(c["kw"].get("sparse"))
    KC.check_case(name, result)
    KC.check_model(name, result, ulps=2)
    n_ref = c["n"] if c["fn"] == "rec" else c["n_ref"]
    k, _, width = KC.plan(c["fn"], c["n"], n_ref, KC.kwargs(name))
    assert ("dense" in on_sim.calls) == (k >= n_ref - width) and ("emit" in on_sim.calls) != ("dense" in on_sim.calls)
    if on_sim.selects:
        rows, tile, k_list, n = on_sim.selects[0]
        assert (rows, tile) == c["geometry"] and geometry(rows, tile, k_list, n)["lds"] > 0


@pytest.mark.parametrize("name", list(KC.TIES))
def test_exact_ties_equal_the_model_on_the_host(name, on_sim):
    KC.check_model(name, KC.call(G, name), ulps=2)


@pytest.mark.parametrize("name", [n for n, c in KC.CASES.items() if c["geometry"] != (0, 0)])
def test_forced_geometry_equals_the_default_geometry_on_the_host(name, on_sim):
    forced, default = (np.ascontiguousarray(KC.dense(KC.call(G, name, geometry=g))) for g in (None, (0, 0)))
    assert on_sim.selects[0][:2] == KC.CASES[name]["geometry"] and on_sim.selects[1][:2] == (0, 0)
    assert forced.dtype == default.dtype and np.array_equal(forced.view(np.uint8), default.view(np.uint8))


def test_sparse_route_takes_no_matrix_sized_buffer_on_the_host(on_sim):
    rng = np.random.default_rng(77)
    x = rng.standard_normal((3, 300))
    G.recurrence_matrix(x, k=4, width=2, mode="affinity", sparse=True)
    assert "dense" not in on_sim.calls and SimSession.scratch_bytes < 300 * (4 + 1) * 64 < 8 * 300 * 300


def test_median_is_numpy_s_nanmedian_on_the_host():
    rng = np.random.default_rng(78)
    for n in (1, 2, 3, 10, 257, 5000):
        v = rng.standard_normal(n) ** 2
        v[rng.random(n) < 0.2] = np.nan
        v[rng.random(n) < 0.05] = 0.0
        if np.isnan(v).all():
            v[0] = 1.0
        work = np.zeros(8, np.int64)
        fn = sim_lib().knnsim_median
        fn.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
        fn(v.ctypes.data, n, work.ctypes.data)
        assert work.view(np.float64)[1] == np.nanmedian(v) and work.view(np.int32)[0] == 0, n
    v = np.full(9, np.nan)
    fn(v.ctypes.data, 9, work.ctypes.data)
    assert work.view(np.int32)[0] == _native.Context.KNN_STATUS_EMPTY_GRAPH
