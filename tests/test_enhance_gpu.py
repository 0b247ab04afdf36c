"""segment.path_enhance, the lag transforms, util.shear and feature.stack_memory on the MI355X: bit for bit against the NumPy models of
tests/enhance_cases.py and against tests/golden/enhance.npz (the unmodified reference) under the rule stated there; NumPy and device-tensor
calls must give the same bits, and the input must be left unwritten.

Shapes are the smallest at which the kernels can go wrong (tests/enhance_cases.py): matrices of 3 x 3 and 1 x 6 under filters that fold the
boundary maps several times, every filter shape from 1 x 1 over even and mixed sides, every boundary mode, forced tiles whose halo exceeds the
tile, the default tile plus 3 and twice it plus 3, and one case of 300 x 260 under the documented 51-cell, seven-filter table."""
import numpy as np
import pytest
import scipy.sparse

import enhance_cases as EC
import librosa_amd as L
from librosa_amd import feature as F
from librosa_amd import segment as G
from librosa_amd import sequence as S
from librosa_amd import util as U

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_laid_out(a, layout):
    """The device tensor of ``a``, in the case's memory layout."""
    return _dev(a.T).T if layout == "fortran" else _dev(a)


def _golden(key, like):
    g = EC.load()[0][key]
    return g.view(np.bool_) if like.dtype == np.bool_ else g


# ---- path_enhance ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EC.PE_CASES))
def test_path_enhance_equals_the_model_and_the_reference(name):
    c = EC.PE_CASES[name]
    R = EC.pe_input(name)
    given = EC.laid_out(R.copy(), c["layout"])
    with np.errstate(all="ignore"):
        result = EC.pe_call(G, name, R=given)
    assert isinstance(result, np.ndarray) and result.dtype == R.dtype and result.shape == R.shape
    assert EC.same_bits(given, R), "the input was written"
    assert EC.same_bits(result, EC.pe_model(name)), f"{name}: max difference {np.nanmax(np.abs(result.astype(np.float64) - EC.pe_model(name).astype(np.float64)))}"
    EC.check_against_golden(name, result)


@pytest.mark.parametrize("name", list(EC.PE_CASES))
def test_path_enhance_device_tensor_gives_the_bits_of_the_numpy_call(name):
    import torch

    c = EC.PE_CASES[name]
    R = EC.pe_input(name)
    t = _dev_laid_out(R, c["layout"])
    assert t.is_contiguous() == (c["layout"] == "plain")
    before = t.clone()
    result = EC.pe_call(G, name, R=t)
    assert torch.is_tensor(result) and result.device == t.device and result.dtype == t.dtype and tuple(result.shape) == R.shape
    assert EC.same_bits(before.cpu().numpy(), t.cpu().numpy()), "the input was written"
    assert EC.same_bits(result.cpu().numpy(), EC.pe_model(name))


@pytest.mark.parametrize("name", [n for n, c in EC.PE_CASES.items() if c["geometry"] != (0, 0)])
def test_forced_geometry_equals_the_default_geometry(name):
    forced, default = (EC.pe_call(G, name, geometry=g) for g in (None, (0, 0)))
    assert EC.same_bits(forced, default)


@pytest.mark.parametrize("tile", [(4, 16), (1, 16), (3, 32), (16, 64), (64, 64), (256, 16)])
def test_every_tile_shape_gives_the_same_bits(tile):
    name = "tile_8x32_n21"
    assert EC.same_bits(EC.pe_call(G, name, geometry=tile), EC.pe_model(name))


def test_a_tile_that_does_not_fit_is_refused():
    with pytest.raises(L.ParameterError, match="ENHANCE_ROWS=64, ENHANCE_COLS=64.*must fit ENHANCE_LDS_MAX=163840 bytes"):
        EC.pe_call(G, "limit", case=EC.PE_LIMIT_OK, geometry=(64, 64))
    for tile in ((0, 16), (4, 8), (300, 16)):
        with pytest.raises(L.ParameterError, match="rows 1 .. 256, cols 16, 32 or 64"):
            EC.pe_call(G, "fold_3x3_n5", geometry=tile)


def test_the_limit_is_served_and_one_over_it_is_refused():
    """A pure diagonal of n cells reaches over n - 1 rows and columns: ENHANCE_MAX_REACH + 1 cells run (at the smallest tile), one more is refused
    with a text that states the limit."""
    c = EC.PE_LIMIT_OK
    R = EC.pe_input("limit", c)
    result = EC.pe_call(G, "limit", R=R, case=c)
    K = L.filters.diagonal_filter("hann", c["n"])
    assert K.shape == (EC.MAX_REACH + 1,) * 2
    assert EC.same_bits(result, np.clip(EC.convolve_model(R, K), 0, None))
    with pytest.raises(L.ParameterError) as e:
        EC.pe_call(G, "limit", R=R, case=EC.PE_LIMIT_OVER)
    assert str(e.value) == (f"path_enhance: the widest of the filters spans {EC.MAX_REACH + 2} cells, above ENHANCE_MAX_REACH + 1 = {EC.MAX_REACH + 1}: its halo does not fit the LDS "
                            "next to a tile")


def test_the_c_entry_point_checks_the_reach_itself():
    """lra_path_enhance_exec derives the halo from the taps it is given and refuses a tap outside LRA_ENHANCE_MAX_REACH: no table reaches LDS it did
    not stage."""
    from librosa_amd import _arrays, _native

    R = np.zeros((4, 4))
    for dr, dc in ((EC.MAX_REACH + 1, 0), (0, -EC.MAX_REACH - 1), (70, 0)):
        taps = np.array([(dr, dc, 1.0), (-60, 0, 1.0)], dtype=_native.Context.ENHANCE_TAP)
        sess = _arrays.Session(R)
        try:
            with pytest.raises(L.ParameterError, match="LRA_ENHANCE_MAX_REACH = 124"):
                sess.ctx.path_enhance_exec(sess.input_raw(R, np.float64), np.float64, 1, 4, 4, taps, [0, 2], 0, 0.0, True, 0, 0, sess.scratch(1024), sess.scratch(128))
        finally:
            sess.close()


# ---- the lag transforms and shear --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", EC.LAG_DTYPES)
@pytest.mark.parametrize("t", EC.LAG_T)
def test_lag_transforms(t, dtype):
    for pad in (True, False):
        for axis in EC.LAG_AXES:
            name = f"t{t}_{dtype}_pad{int(pad)}_axis{axis}"
            x = EC.lag_input(name)
            before = x.copy()
            lag = G.recurrence_to_lag(x, pad=pad, axis=axis)
            want = EC.rec_to_lag_model(x, pad, axis)
            assert isinstance(lag, np.ndarray) and EC.same_bits(lag, want) and EC.same_bits(lag, _golden(f"lag/{name}", x)), name
            back = G.lag_to_recurrence(lag, axis=axis)
            assert EC.same_bits(back, x) and EC.same_bits(x, before), name
            d = _dev(x)
            lag_d = G.recurrence_to_lag(d, pad=pad, axis=axis)
            assert lag_d.dtype == d.dtype and lag_d.is_cuda and EC.same_bits(lag_d.cpu().numpy(), want), name
            assert EC.same_bits(G.lag_to_recurrence(lag_d, axis=axis).cpu().numpy(), x) and EC.same_bits(d.cpu().numpy(), x), name


def test_lag_of_a_non_contiguous_view():
    x = EC.lag_input("t33_float64_pad1_axis1")
    assert EC.same_bits(G.recurrence_to_lag(np.asfortranarray(x)), EC.rec_to_lag_model(x, True, 1))
    assert EC.same_bits(G.recurrence_to_lag(_dev(x.T).T).cpu().numpy(), EC.rec_to_lag_model(x, True, 1))


@pytest.mark.parametrize("name", list(EC.SHEAR_CASES))
def test_shear(name):
    c = EC.SHEAR_CASES[name]
    x = EC.shear_input(name)
    want = EC.shear_model(x, c["factor"], c["axis"])
    assert EC.same_bits(U.shear(x, factor=c["factor"], axis=c["axis"]), want) and EC.same_bits(want, _golden(f"shear/{name}", x))
    assert EC.same_bits(U.shear(_dev(x), factor=c["factor"], axis=c["axis"]).cpu().numpy(), want)


@pytest.mark.parametrize("fmt", EC.SPARSE_FORMATS)
def test_scipy_sparse_agrees_with_the_device(fmt):
    x = EC.lag_input("t33_float64_pad1_axis1")
    x[x < 0.7] = 0
    sp = scipy.sparse.coo_array(x).asformat(fmt)
    for axis in EC.LAG_AXES:
        lag = G.recurrence_to_lag(sp, axis=axis)
        assert lag.format == fmt and EC.same_bits(lag.toarray(), G.recurrence_to_lag(x, axis=axis))
        assert EC.same_bits(G.lag_to_recurrence(lag, axis=axis).toarray(), x)


@pytest.mark.parametrize("refusal", ["lag_non_square", "lag_three_dims", "rec_bad_axis", "rec_bad_shape", "rec_bad_shape_axis0"])
def test_lag_refusals_on_device_tensors(refusal):
    import torch

    shapes = {"lag_non_square": (3, 4), "lag_three_dims": (3, 3, 3), "rec_bad_axis": (4, 4), "rec_bad_shape": (5, 3), "rec_bad_shape_axis0": (8, 4)}
    x = torch.zeros(shapes[refusal], device="cuda")
    with pytest.raises(L.ParameterError) as e:
        if refusal.startswith("lag"):
            G.recurrence_to_lag(x)
        else:
            G.lag_to_recurrence(x, axis=2 if refusal == "rec_bad_axis" else 0 if refusal.endswith("axis0") else -1)
    assert str(e.value) == EC.load()[1]["refusals"][refusal]


def _roll_rows(x, shift=2):
    """A pure-Python filter: the rows rolled, on whatever kind of matrix it is given."""
    return x[[(r - shift) % x.shape[0] for r in range(x.shape[0])]]


@pytest.mark.parametrize("pad", [True, False])
def test_timelag_filter(pad):
    x = EC.lag_input("t33_float32_pad1_axis1")
    wrapped = G.timelag_filter(_roll_rows, pad=pad)
    want = EC.lag_to_rec_model(_roll_rows(EC.rec_to_lag_model(x, pad, 1)), 1)
    assert EC.same_bits(wrapped(x), want)
    got = wrapped(_dev(x))
    assert got.is_cuda and EC.same_bits(got.cpu().numpy(), want)
    indexed = G.timelag_filter(lambda shift, m: _roll_rows(m, shift), pad=pad, index=1)
    assert EC.same_bits(indexed(5, x), EC.lag_to_rec_model(_roll_rows(EC.rec_to_lag_model(x, pad, 1), 5), 1))


# ---- stack_memory ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EC.STACK_CASES))
def test_stack_memory(name):
    c = EC.STACK_CASES[name]
    x = EC.stack_input(name)
    before = x.copy()
    want = EC.stack_model(x, c["n_steps"], c["delay"], **c["kw"])
    result = EC.stack_call(F, name, data=x)
    assert isinstance(result, np.ndarray) and EC.same_bits(result, want) and EC.same_bits(result, _golden(f"stack/{name}", x)) and EC.same_bits(x, before)
    d = _dev(x)
    on_device = EC.stack_call(F, name, data=d)
    assert on_device.is_cuda and on_device.dtype == d.dtype and EC.same_bits(on_device.cpu().numpy(), want) and EC.same_bits(d.cpu().numpy(), x)


def test_stack_memory_of_a_non_contiguous_view():
    x = EC.stack_input("reflect_d3_s10")
    want = EC.stack_model(x, 10, 3, mode="reflect")
    assert EC.same_bits(F.stack_memory(np.asfortranarray(x), n_steps=10, delay=3, mode="reflect"), want)
    assert EC.same_bits(F.stack_memory(_dev(x.T).T, n_steps=10, delay=3, mode="reflect").cpu().numpy(), want)


@pytest.mark.parametrize("refusal", ["stack_n_steps", "stack_delay", "stack_no_columns"])
def test_stack_refusals_on_device_tensors(refusal):
    import torch

    x = torch.zeros((3, 0) if refusal == "stack_no_columns" else (4, 4), device="cuda")
    with pytest.raises(L.ParameterError) as e:
        F.stack_memory(x, **({"n_steps": 0} if refusal == "stack_n_steps" else {"delay": 0} if refusal == "stack_delay" else {}))
    assert str(e.value) == EC.load()[1]["refusals"][refusal]


# ---- the documented chain, on device tensors -----------------------------------------------------------------------------------------------------------------
def test_chain_stays_on_the_device():
    """chroma_cqt-sized features -> stack_memory -> recurrence_matrix(affinity, self) -> path_enhance -> rqa: the device-tensor chain gives the
    score and the path of the NumPy chain."""
    import torch

    rng = np.random.default_rng(20)
    chroma = rng.random((12, 160)) + np.tile(rng.random((12, 40)), 4)   # (a repeated section: there is a path to find)

    def chain(x):
        stack = F.stack_memory(x, n_steps=10, delay=3)
        rec = G.recurrence_matrix(stack, mode="affinity", self=True)
        smooth = G.path_enhance(rec, 21, window="hann", n_filters=7)
        lag = G.recurrence_to_lag(smooth)
        score, path = S.rqa(smooth)
        return stack, rec, smooth, lag, score, path

    host = chain(chroma)
    device = chain(_dev(chroma))
    assert host[0].shape == (120, 160) and host[2].shape == (160, 160) and host[3].shape == (320, 160) and len(host[5]) > 1
    for h, d in zip(host, device):
        assert isinstance(h, np.ndarray) and torch.is_tensor(d) and d.is_cuda
        assert EC.same_bits(d.cpu().numpy(), h)
