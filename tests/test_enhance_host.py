"""Host side of segment.path_enhance, the lag transforms, util.shear and feature.stack_memory: the NumPy models of tests/enhance_cases.py against
tests/golden/enhance.npz (the unmodified reference), filters.diagonal_filter against the reference's tables bit for bit, the tap table's order
and offsets against scipy.ndimage.convolve itself, and every argument check with its text.  No GPU."""
import inspect
import os

import numpy as np
import pytest
import scipy.ndimage
import scipy.sparse

import enhance_cases as EC
import librosa_amd as L
from librosa_amd import _native
from librosa_amd import feature as F
from librosa_amd import filters
from librosa_amd import segment as G
from librosa_amd import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(key, like):
    g = EC.load()[0][key]
    return g.view(np.bool_) if like.dtype == np.bool_ else g


# ---- models against the reference ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EC.PE_CASES))
def test_convolution_model_equals_the_reference(name):
    assert not EC.load()[1]["pe"][name]["deviates"]
    assert EC.same_bits(EC.pe_model(name), EC.load()[0][f"pe/{name}"])


def test_lag_models_equal_the_reference():
    for name, c in EC.LAG_CASES.items():
        x = EC.lag_input(name)
        lag = EC.rec_to_lag_model(x, c["pad"], c["axis"])
        assert EC.same_bits(lag, _golden(f"lag/{name}", x)), name
        assert EC.same_bits(EC.lag_to_rec_model(lag, c["axis"]), x), name


def test_shear_model_equals_the_reference():
    for name, c in EC.SHEAR_CASES.items():
        x = EC.shear_input(name)
        assert EC.same_bits(EC.shear_model(x, c["factor"], c["axis"]), _golden(f"shear/{name}", x)), name


def test_stack_model_equals_the_reference():
    for name, c in EC.STACK_CASES.items():
        x = EC.stack_input(name)
        assert EC.same_bits(EC.stack_model(x, c["n_steps"], c["delay"], **c["kw"]), _golden(f"stack/{name}", x)), name


# ---- filters.diagonal_filter -----------------------------------------------------------------------------------------------------------------------------
def test_diagonal_filter_equals_the_reference_tables():
    arrays, meta = EC.load()
    assert len(meta["filters"]) >= 15
    for i, f in enumerate(meta["filters"]):
        window = tuple(f["window"]) if isinstance(f["window"], list) else f["window"]
        K = filters.diagonal_filter(window, f["n"], **f["kw"])
        assert K.dtype == np.float64 and EC.same_bits(K, arrays[f"filter/{i}"]), f
        cached = filters.diagonal_filter_cached(window, f["n"], **f["kw"])
        assert EC.same_bits(cached, K) and not cached.flags.writeable
        assert filters.diagonal_filter_cached(window, f["n"], **f["kw"]) is cached
    assert str(inspect.signature(filters.diagonal_filter)) == "(window, n, *, slope=1.0, angle=None, zero_mean=False)"
    assert EC.same_bits(filters.diagonal_filter_cached(np.ones(4), 4, slope=2.0), filters.diagonal_filter(np.ones(4), 4, slope=2.0))   # (unhashable window)


def test_documented_filters_are_sparse():
    """n = 51, seven filters, ratio 2: 51 to 65 cells square, about 3 000 weights in all."""
    taps, starts = G._filter_taps([filters.diagonal_filter("hann", 51, slope=r) for r in np.logspace(-1, 1, num=7, base=2)])
    assert starts[0] == 0 and starts[-1] == taps.size and 2500 < taps.size < 3500
    assert max(np.abs(taps["dr"]).max(), np.abs(taps["dc"]).max()) <= 32 <= G.ENHANCE_MAX_REACH


# ---- the tap table ---------------------------------------------------------------------------------------------------------------------------------------
def test_tap_table_order_and_offsets_by_hand():
    odd = np.arange(1.0, 10.0).reshape(3, 3)
    taps, starts = G._filter_taps([odd])
    assert list(starts) == [0, 9] and taps.dtype == _native.Context.ENHANCE_TAP and taps.dtype.itemsize == 16
    assert [tuple(t) for t in taps[:4]] == [(-1, -1, 9.0), (-1, 0, 8.0), (-1, 1, 7.0), (0, -1, 6.0)] and tuple(taps[-1]) == (1, 1, 1.0)
    even = np.array([[1.0, 2.0], [3.0, 4.0]])
    taps, starts = G._filter_taps([even])
    assert [tuple(t) for t in taps] == [(0, 0, 4.0), (0, 1, 3.0), (1, 0, 2.0), (1, 1, 1.0)]
    holes = np.array([[0.0, 1.0, 0.0], [np.nan, 0.0, 1e-17], [2.0, 0.0, -3.0]])   # zeros, a NaN and rounding noise are left out, as scipy.ndimage's footprint leaves them out
    taps, starts = G._filter_taps([holes, odd], origin=(0, 0))
    assert list(starts) == [0, 3, 12] and [tuple(t) for t in taps[:3]] == [(-1, -1, -3.0), (-1, 1, 2.0), (1, 0, 1.0)]


@pytest.mark.parametrize("side", [(3, 3), (2, 2), (4, 4), (5, 5), (6, 6), (1, 1)])
@pytest.mark.parametrize("origin", [(0, 0), (1, -1), (-1, 0), (0, 1)])
def test_tap_table_is_scipy_s_sum(side, origin):
    rng = np.random.default_rng(side[0] * 10 + origin[0] + 3 * origin[1])
    K = rng.random(side) - 0.3
    K[rng.random(side) < 0.3] = 0.0
    R = rng.random((5, 7))
    for m, o in zip(side, origin):
        conv_o = -o - (0 if m & 1 else 1)
        if conv_o < -(m // 2) or conv_o > (m - 1) // 2:
            with pytest.raises(L.ParameterError, match="Invalid origin"):
                G._filter_taps([K], origin)
            with pytest.raises(ValueError, match="nvalid origin"):
                scipy.ndimage.convolve(R, K, origin=origin)
            return
    taps, _ = G._filter_taps([K], origin)
    assert [tuple(t) for t in taps] == EC.taps_of(K, origin)
    for mode in ("reflect", "constant", "nearest", "mirror", "wrap"):
        want = scipy.ndimage.convolve(R, K, mode=mode, cval=0.25, origin=origin)
        assert EC.same_bits(EC.convolve_model(R, K, mode, 0.25, origin), want), (mode, side, origin)


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EC.refusals()))
def test_refusals_carry_the_reference_text(name):
    with pytest.raises(L.ParameterError) as e:
        EC.refusals()[name](L)
    assert str(e.value) == EC.load()[1]["refusals"][name]


def test_signatures_are_the_reference_s():
    assert str(inspect.signature(G.path_enhance)) == "(R, n, *, window='hann', max_ratio=2.0, min_ratio=None, n_filters=7, zero_mean=False, clip=True, **kwargs)"
    assert str(inspect.signature(G.recurrence_to_lag)) == "(rec, *, pad=True, axis=-1)"
    assert str(inspect.signature(G.lag_to_recurrence)) == "(lag, *, axis=-1)"
    assert str(inspect.signature(G.timelag_filter)) == "(function, pad=True, index=0)"
    assert str(inspect.signature(U.shear)) == "(X, *, factor=1, axis=-1)"
    assert str(inspect.signature(F.stack_memory)) == "(data, *, n_steps=2, delay=1, **kwargs)"
    for name in ("path_enhance", "recurrence_to_lag", "lag_to_recurrence", "timelag_filter"):
        assert name in G.ENHANCE_NAMES and callable(getattr(L.segment, name)) and getattr(L.segment, name) is getattr(G, name)
    assert "stack_memory" in F.__all__ and "shear" in U.__all__ and "diagonal_filter" in filters.__all__


R44 = np.zeros((4, 4))


@pytest.mark.parametrize("call, text", [
    (lambda: G.path_enhance(R44, 3, n_filters=0), "n_filters=0 must be a positive integer"),
    (lambda: G.path_enhance(R44, 3, n_filters=None), "n_filters=None must be a positive integer"),
    (lambda: G.path_enhance(R44 > 0, 3), "R must be float32 or float64, given dtype=bool: convert it"),
    (lambda: G.path_enhance(R44.astype(np.int32), 3), "R must be float32 or float64, given dtype=int32: convert it"),
    (lambda: G.path_enhance(R44.astype(np.float16), 3), "R must be float32 or float64, given dtype=float16: convert it"),
    (lambda: G.path_enhance(R44.astype(np.complex128), 3), "R must be real-valued, given dtype=complex128"),
    (lambda: G.path_enhance(scipy.sparse.csr_array(R44), 3), "path_enhance does not support sparse input"),
    (lambda: G.path_enhance(np.zeros(4), 3), "R must have at least 2 dimensions, given R.shape=(4,)"),
    (lambda: G.path_enhance(np.zeros((0, 4)), 3), "R is empty: R.shape=(0, 4)"),
    (lambda: G.path_enhance(R44, 3, output=np.float32), "the keyword argument 'output' of scipy.ndimage.convolve is not served"),
    (lambda: G.path_enhance(R44, 3, axes=(0, 1)), "the keyword argument 'axes' of scipy.ndimage.convolve is not served"),
    (lambda: G.path_enhance(R44, 3, mode=["reflect", "wrap"]), "the keyword argument 'mode' must be one string for all axes"),
    (lambda: G.path_enhance(R44, 3, mode="symmetric"), "mode='symmetric' is not a boundary mode of scipy.ndimage.convolve"),
    (lambda: G.path_enhance(R44, 3, origin=2), "Invalid origin; origin must satisfy"),
    (lambda: G.path_enhance(R44, 3, origin=(0, -2)), "Invalid origin; origin must satisfy"),
    (lambda: G.path_enhance(R44, 3, origin=(0, 0, 0)), "origin must be an integer or a pair, given 3 entries"),
    (lambda: G.path_enhance(np.zeros((2, 4, 4)), 3, origin=1), "Invalid origin; origin must satisfy"),
    (lambda: EC.pe_call(G, "over", case=EC.PE_LIMIT_OVER), f"the widest of the filters spans {EC.MAX_REACH + 2} cells, above ENHANCE_MAX_REACH + 1 = {EC.MAX_REACH + 1}"),
    (lambda: G.path_enhance(R44, 120, max_ratio=3.0), "above ENHANCE_MAX_REACH + 1 = 125"),
    (lambda: U.shear(np.zeros((2, 2, 2))), "Input must be 2D. Provided shape=(2, 2, 2)."),
    (lambda: U.shear(np.zeros((2, 2), dtype=np.complex128)), "shear moves elements of 1, 2, 4 or 8 bytes"),
    (lambda: F.stack_memory(R44, mode="mean"), "mode='mean' is not served on the device: one of constant, edge, reflect, symmetric, wrap"),
    (lambda: F.stack_memory(R44, mode="linear_ramp"), "mode='linear_ramp' is not served on the device"),
    (lambda: F.stack_memory(R44, mode=lambda *a: None), "is not served on the device"),
    (lambda: F.stack_memory(R44, stat_length=2), "the keyword argument 'stat_length' of np.pad is not served"),
    (lambda: F.stack_memory(R44, mode="reflect", reflect_type="odd"), "the keyword argument 'reflect_type' of np.pad is not served"),
    (lambda: F.stack_memory(R44, constant_values=[1, 2]), "constant_values must be a scalar on the device, given shape=(2,)"),
    (lambda: F.stack_memory(R44, mode="edge", constant_values=1), "constant_values goes with mode='constant'"),
])
def test_argument_checks(call, text):
    """Checks that need no device: a complex shear and the device-side ones are refused before any launch."""
    with pytest.raises(L.ParameterError) as e:
        call()
    assert text in str(e.value), str(e.value)


def test_torch_sparse_is_refused():
    torch = pytest.importorskip("torch")
    s = torch.eye(3).to_sparse()
    for call in (lambda: U.shear(s), lambda: G.recurrence_to_lag(s), lambda: G.lag_to_recurrence(s)):
        with pytest.raises(L.ParameterError, match="does not take a torch sparse tensor"):
            call()
    with pytest.raises(L.ParameterError, match="does not support sparse input"):
        G.path_enhance(s, 3)


# ---- scipy.sparse on the host, as the reference does -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", EC.SPARSE_FORMATS)
@pytest.mark.parametrize("axis", EC.LAG_AXES)
@pytest.mark.parametrize("pad", [True, False])
def test_scipy_sparse_lag_transforms(fmt, axis, pad):
    for t in (1, 2, 5, 33):
        name = f"t{t}_float64_pad{int(pad)}_axis{axis}"
        x = EC.lag_input(name)
        x[x < 0.6] = 0
        sp = scipy.sparse.coo_array(x).asformat(fmt)
        data_before = sp.data.copy()
        lag = G.recurrence_to_lag(sp, pad=pad, axis=axis)
        assert scipy.sparse.issparse(lag) and lag.format == fmt and lag.dtype == x.dtype
        assert np.array_equal(lag.toarray(), EC.rec_to_lag_model(x, pad, axis)), (t, fmt)
        back = G.lag_to_recurrence(lag, axis=axis)
        assert back.format == fmt and np.array_equal(back.toarray(), x) and np.array_equal(sp.data, data_before)
        sheared = U.shear(sp, factor=3, axis=axis)
        assert sheared.format == fmt and np.array_equal(sheared.toarray(), EC.shear_model(x, 3, axis))
    m = scipy.sparse.csr_matrix(x)
    assert isinstance(U.shear(m, factor=-1), scipy.sparse.spmatrix)


# ---- the C surface -----------------------------------------------------------------------------------------------------------------------------------------
def test_abi_and_constants():
    from librosa_amd import build

    assert "enhance_inst" in build.UNITS
    header = open(os.path.join(ROOT, "include", "librosa_amd.h")).read()
    unit = open(os.path.join(ROOT, "librosa_amd", "csrc", "lra_enhance_inst.hip")).read()   # the unit that defines the entry points, beside their kernels
    api = open(os.path.join(ROOT, "librosa_amd", "csrc", "lra_api.hip")).read()
    for name in ("lra_enhance_lds_bytes", "lra_path_enhance_exec", "lra_shear_exec", "lra_stack_memory_exec"):
        assert name in _native.SIGNATURES and name in header and name in unit and name not in api
    C = _native.Context
    assert f"#define LRA_ENHANCE_MAX_REACH {C.ENHANCE_MAX_REACH}" in header and C.ENHANCE_MAX_REACH == G.ENHANCE_MAX_REACH == EC.MAX_REACH
    assert "#define LRA_ENHANCE_LDS_MAX (160 * 1024)" in header and C.ENHANCE_LDS_MAX == 160 * 1024
    for word, code in C.ENHANCE_MODES.items():
        assert f"#define LRA_ENHANCE_{word.upper()} {code}" in header
    for word, code in C.STACK_MODES.items():
        assert f"#define LRA_STACK_{word.upper()} {code}" in header
    assert (G.ENHANCE_ROWS, G.ENHANCE_COLS) == (0, 0) and "4.6r" in G.path_enhance.__doc__ and "segment.path_enhance" in L.__doc__
    assert C.enhance_table_bytes(3187, 7) == 32 + 16 * 3187


def test_geometry_arithmetic():
    """lra_enhance_lds_bytes is host arithmetic: the documented call runs at the first choice, the longest reach is served, and a forced tile
    that does not fit is refused."""
    lib = _native.load_library()
    f = lib.lra_enhance_lds_bytes
    assert f(0, 0, 62, 62) == 8 * (64 + 62) * (64 + 62) == f(*EC.DEFAULT_TILE, 62, 62) <= 160 * 1024
    assert f(0, 0, 64, 64) == 8 * 128 * 128
    assert f(0, 0, EC.MAX_REACH, EC.MAX_REACH) == f(16, 16, EC.MAX_REACH, EC.MAX_REACH) == 8 * 140 * 144 and f(4, 16, EC.MAX_REACH, EC.MAX_REACH) == 8 * 128 * 144
    assert f(0, 0, 100, 100) == f(32, 32, 100, 100) == 8 * 132 * 132 and f(32, 64, 100, 100) == 0
    assert f(8, 16, 100, 100) == 8 * 108 * 144   # (16 columns: the pitch is 16 mod 32 doubles)
    assert f(64, 64, 100, 100) == 0 and f(16, 64, 0, 0) == 8 * 16 * 64
    for rows, cols in ((0, 16), (16, 0), (257, 16), (4, 8), (4, 48), (128, 64), (-1, 16)):
        assert f(rows, cols, 4, 4) == 0, (rows, cols)
    assert f(256, 16, 0, 0) > 0 and f(64, 64, 0, 0) > 0 and f(4, 16, -1, 0) == 0
