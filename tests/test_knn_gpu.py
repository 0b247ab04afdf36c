"""segment.recurrence_matrix and cross_similarity on the MI355X against tests/golden/knn.npz (the unmodified reference) under the rule of
tests/knn_cases.py -- the pattern exactly, values within the reference's own recorded deviation plus the bound of a direct sum -- and against the
NumPy model, bit for bit, where the reference cannot judge (exact ties).

Shapes are the smallest at which the kernels can go wrong (tests/knn_cases.py): t = 5, 7, 9 at the largest legal width, 33, 70, and the shipped
tile plus three and twice it plus three; the cross shapes from 1 x 1 to 70 x 33; row blocks and candidate tiles forced to (1, 4), (4, 8), (8, 16)
with k one under, at and one over the tile; every mode with sym and self, every bandwidth form, sparse and full both ways, float32 and integer
features, exact duplicates.  One case at t = 1500 has 375 row blocks of 12 tiles and bounds the memory the sparse route takes."""
import numpy as np
import pytest

import knn_cases as KC
import librosa_amd as L
from librosa_amd import segment as G
from librosa_amd import sequence as S

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", list(KC.CASES))
def test_numpy_call_matches_the_reference(name):
    entry = KC.load()[1]["cases"][name]
    if "refused" in entry:
        with pytest.raises(L.ParameterError) as e:
            KC.call(G, name)
        assert str(e.value) == entry["refused"]
        return
    result = KC.call(G, name)
    assert (type(result).__name__ == "csc_array") if KC.CASES[name]["kw"].get("sparse") else isinstance(result, np.ndarray)
    KC.check_case(name, result)
    KC.check_model(name, result, ulps=2)


@pytest.mark.parametrize("name", list(KC.TIES))
def test_exact_ties_equal_the_model(name):
    KC.check_model(name, KC.call(G, name), ulps=2)


@pytest.mark.parametrize("name", [n for n, c in KC.CASES.items() if c["geometry"] != (0, 0)])
def test_forced_geometry_equals_the_default_geometry(name):
    forced, default = (np.ascontiguousarray(KC.dense(KC.call(G, name, geometry=g))) for g in (None, (0, 0)))
    assert forced.dtype == default.dtype and np.array_equal(forced.view(np.uint8), default.view(np.uint8))


@pytest.mark.parametrize("name", list(KC.refusals()))
def test_refusals_carry_the_reference_text(name):
    with pytest.raises(L.ParameterError) as e:
        KC.refusal_call(G, name)
    assert str(e.value) == KC.load()[1]["refusals"][name]
    if name in ("no_neighbors", "empty_graph"):
        with pytest.raises(L.ParameterError) as e:
            KC.refusal_call(G, name, wrap=_dev)
        assert str(e.value) == KC.load()[1]["refusals"][name]


TENSOR_CASES = [n for i, (n, c) in enumerate(KC.CASES.items()) if "refused" not in KC.load()[1]["cases"][n] and (i % 4 == 0 or c["geometry"] != (0, 0) or c["dtype"] != "float64" or c["layout"] != "plain")]


@pytest.mark.parametrize("name", TENSOR_CASES)
def test_device_tensor_gives_the_bits_of_the_numpy_call(name):
    import torch

    host = KC.call(G, name)
    kept = []

    def wrap(a):
        kept.append((_dev(a), _dev(a)))
        return kept[-1][0]

    result = KC.call(G, name, wrap=wrap)
    assert isinstance(result, torch.Tensor) and result.is_cuda
    if KC.CASES[name]["kw"].get("sparse"):
        assert result.layout == torch.sparse_csc and result.ccol_indices().dtype == torch.int32 and result.row_indices().dtype == torch.int32
        assert np.array_equal(result.ccol_indices().cpu().numpy(), host.indptr) and np.array_equal(result.row_indices().cpu().numpy(), host.indices)
        assert np.array_equal(result.values().cpu().numpy(), host.data, equal_nan=True) and result.values().dtype == getattr(torch, host.dtype.name)
        # the sparse tensor densifies to the dense result of the same call
        assert np.array_equal(result.to_dense().cpu().numpy(), host.toarray(), equal_nan=True)
    else:
        assert result.layout == torch.strided and result.dtype == getattr(torch, host.dtype.name) and tuple(result.shape) == host.shape
        assert np.array_equal(result.cpu().numpy(), host, equal_nan=True)
    for given, copy in kept:
        assert torch.equal(given, copy), "the input was written"


def test_sparse_tensor_densifies_to_the_dense_result():
    import torch

    x = _dev(np.random.default_rng(11).standard_normal((12, 70)))
    for mode in KC.MODES:
        for kw in (dict(), dict(sym=True, self=True), dict(full=True)):
            dense = G.recurrence_matrix(x, mode=mode, width=2, **kw)
            sparse = G.recurrence_matrix(x, mode=mode, width=2, sparse=True, **kw)
            assert sparse.is_cuda and sparse.layout == torch.sparse_csc and np.array_equal(sparse.to_dense().cpu().numpy(), dense.cpu().numpy())


def test_the_chain_into_rqa_stays_on_the_device():
    import torch

    rng = np.random.default_rng(12)
    a, b = rng.standard_normal((12, 90)), rng.standard_normal((12, 70))
    xsim = G.cross_similarity(_dev(a), _dev(b), mode="affinity")
    assert isinstance(xsim, torch.Tensor) and xsim.is_cuda and tuple(xsim.shape) == (70, 90)
    score, path = S.rqa(xsim)
    assert score.is_cuda and path.is_cuda
    h_score, h_path = S.rqa(G.cross_similarity(a, b, mode="affinity"))
    assert np.array_equal(score.cpu().numpy(), h_score) and np.array_equal(path.cpu().numpy(), h_path) and len(h_path) > 0


_big = {}


def big():
    """t = 1500, d = 12, the default k = 78: 375 row blocks of 12 tiles; the model, computed once."""
    if not _big:
        _big["x"] = np.random.default_rng(13).standard_normal((12, 1500))
        c = dict(fn="rec", metric="euclidean")
        for mode in ("distance", "connectivity"):
            _big[mode] = KC.model(c, _big["x"], None, dict(mode=mode, width=3, sym=mode == "connectivity"))[0]
    return _big


@pytest.mark.parametrize("mode", ["distance", "connectivity"])
def test_many_row_blocks_and_tiles_equal_the_model(mode):
    want = big()[mode]
    got = G.recurrence_matrix(big()["x"], mode=mode, width=3, sym=mode == "connectivity", sparse=mode == "distance")
    got = KC.dense(got)
    assert got.dtype == want.dtype and np.array_equal(got, want)


def test_the_sparse_route_takes_no_matrix_sized_buffer():
    import torch

    t, k = 1500, 78
    x = _dev(big()["x"])
    G.recurrence_matrix(x, mode="affinity", width=3, sparse=True)   # (the context, the library and torch's pools exist after this)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = G.recurrence_matrix(x, mode="affinity", width=3, sparse=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    # count, index, distance, keep, the statistics, the compressed arrays and the features: under 64 bytes per list slot, against 8 t^2 for a matrix
    assert out.values().numel() <= t * k and 0 < peak < 64 * t * (k + 1) < 8 * t * t, peak
