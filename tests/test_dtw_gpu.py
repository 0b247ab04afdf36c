"""sequence.dtw and dtw_backtracking on the MI355X against tests/golden/dtw.npz (the unmodified reference), under the two rules of
tests/dtw_cases.py: with a given C, and for dtw_backtracking, D, steps and wp bit-equal; with X and Y, wp equal and D within
delta = (N + M - 1) (max|w_mul| eps_C + 3 ulp(max finite D)) on certified cases.

Shapes are the smallest at which the kernels can go wrong (tests/dtw_cases.py): 1 x 1, one row, one column, 63 x 65, 64 x 64, 65 x 130, 130 x 65
and 129 x 130 around the tile of 64 (a 3 x 3 grid), each with random costs and with integer costs full of exact ties; tiles of 8, 16 and 32 forced
at 20 x 37, 37 x 20 and 65 x 70; step tables with halos of 2, 3 and 8, with 16 steps, with infinite default weights against zero costs; negative
costs; subseq with N < M, N > M and a tall given C; the Sakoe-Chiba band at 40 x 50 and 50 x 40; float32, int32, int64, uint8 and int16 C; the
four metrics at 12 x 130 against 12 x 70, a 1-D pair, a lead shape, float32 features.

Measured on the MI355X (printed per case): every given-C and dtw_backtracking case bit-equal; every X/Y case at the reference's path; worst error
of D per metric: euclidean 5.68e-14 (xy_euclidean, bound 2.16e-11; xy_sub_130x70 1.42e-14, xy_f32 7.11e-15, xy_1d 0), sqeuclidean 5.68e-14 (bound
6.36e-11; xy_s121 2.84e-14), cityblock 0 (bounds 4.77e-11 and 4.54e-11), cosine 1.6e-14 (xy_sub_70x130, bound 3.53e-12; xy_cosine 1.07e-14)."""
import numpy as np
import pytest

import dtw_cases as DC
import librosa_amd as L
from librosa_amd import sequence as S

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", list(DC.CASES))
def test_numpy_call_matches_the_reference(name):
    D, wp, steps = DC.run_case(name, S)
    assert isinstance(D, np.ndarray) and isinstance(wp, np.ndarray) and isinstance(steps, np.ndarray)
    DC.check_case(name, D, wp, steps, report=print)


@pytest.mark.parametrize("name", ["t8_20x37", "t8_37x20", "t16_65x70", "t32_65x70", "s313_t8_66x90", "s8_t8_40x47", "gc_t8_40x50"])
def test_forced_tile_equals_the_default_tile(name):
    for a, b in zip(DC.run_case(name, S), DC.run_case(name, S, tile=0)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("tile", [0, 8, 32])
def test_many_launches_equal_the_model(tile):
    # 257 x 300: a 5 x 5 grid at the default tile, 33 x 38 tiles (70 launches) at tile 8; integer costs, so every tie is exact
    C = np.random.default_rng(4242).integers(0, 3, size=(257, 300)).astype(np.float64)
    mD, mwp, mS = DC.model_dtw(C, {})
    old = S.DTW_TILE
    S.DTW_TILE = tile
    try:
        D, wp, steps = S.dtw(C=C, return_steps=True)
    finally:
        S.DTW_TILE = old
    assert np.array_equal(D, mD) and np.array_equal(steps, mS) and np.array_equal(wp, mwp)


TENSOR_CASES = ["c_1x1_rand", "c_129x130_ints", "c_130x65_rand", "t8_37x20", "s313_66x90", "s16_30x33", "neg_sub_33x70", "sub_70x33", "gc_sub_50x40", "c_f32_20x37", "c_u8_20x37", "c_i64_20x37",
                "xy_cosine", "xy_sub_130x70", "xy_1d", "xy_lead", "xy_f32"]


@pytest.mark.parametrize("name", TENSOR_CASES)
def test_device_tensor_gives_the_bits_of_the_numpy_call(name):
    import torch

    host = DC.run_case(name, S)
    kept = []

    def wrap(a):
        kept.append((_dev(a), _dev(a)))
        return kept[-1][0]

    D, wp, steps = DC.run_case(name, S, wrap=wrap)
    for t, dtype, h in ((D, torch.float64, host[0]), (wp, torch.int64, host[1]), (steps, torch.int32, host[2])):
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and tuple(t.shape) == h.shape
        assert np.array_equal(t.cpu().numpy(), h, equal_nan=True)
    for given, copy in kept:
        assert torch.equal(given, copy), "the input was written"


def test_return_combinations():
    a = DC.inputs("c_63x65_rand")
    D, wp, steps = S.dtw(C=a["C"], return_steps=True)
    only = S.dtw(C=a["C"], backtrack=False)
    assert isinstance(only, np.ndarray) and np.array_equal(only, D)
    D2, wp2 = S.dtw(C=a["C"])
    assert np.array_equal(D2, D) and np.array_equal(wp2, wp)
    D3, steps3 = S.dtw(C=a["C"], backtrack=False, return_steps=True)
    assert np.array_equal(D3, D) and np.array_equal(steps3, steps) and steps3.dtype == np.int32


@pytest.mark.parametrize("name", list(DC.BACKTRACKS))
def test_dtw_backtracking_matches_the_reference(name):
    import torch

    case, kw = DC.BACKTRACKS[name]
    a = DC.inputs(case)
    steps = DC.model(a["C"], a["kw"])[1]
    wp = S.dtw_backtracking(steps, **kw)
    assert isinstance(wp, np.ndarray) and wp.dtype == np.int64 and np.array_equal(wp, DC.load()[0][f"{name}/wp"])
    t, keep = _dev(steps), _dev(steps)
    wpt = S.dtw_backtracking(t, **kw)
    assert isinstance(wpt, torch.Tensor) and wpt.is_cuda and wpt.dtype == torch.int64 and np.array_equal(wpt.cpu().numpy(), wp) and torch.equal(t, keep)


def test_dtw_backtracking_edges():
    steps = np.zeros((4, 2), dtype=np.int32)
    assert S.dtw_backtracking(steps).tolist() == [[3, 1], [2, 0]]   # (the reference's break where an index goes negative)
    steps = np.zeros((6, 9), dtype=np.int32)
    steps[4, 7] = 3
    with pytest.raises(L.ParameterError, match="outside the step table"):
        S.dtw_backtracking(steps)
    with pytest.raises(L.ParameterError, match="outside the step table"):
        S.dtw_backtracking(_dev(steps))


@pytest.mark.parametrize("name", [n for n, r in DC.refusals().items() if r[3]])
def test_status_words_refuse_with_the_reference_text(name):
    fn, args, kw, _ = DC.refusals()[name]
    with pytest.raises(L.ParameterError) as e:
        getattr(S, fn)(*args, **kw)
    assert str(e.value) == DC.load()[1]["refusals"][name]
    with pytest.raises(L.ParameterError) as e:
        getattr(S, fn)(*args, **{k: _dev(v) if k == "C" else v for k, v in kw.items()})
    assert str(e.value) == DC.load()[1]["refusals"][name]


def test_cosine_of_a_zero_vector_is_nan_and_refused():
    X, Y = np.ones((3, 5)), np.ones((3, 70))
    Y[:, 44] = 0.0
    with pytest.raises(L.ParameterError, match="DTW cost matrix C has NaN values"):
        S.dtw(X, Y, metric="cosine")
    with pytest.raises(L.ParameterError, match="DTW cost matrix C has NaN values"):
        S.dtw(_dev(X), _dev(Y), metric="cosine")
