"""Every FIR decimator route and the rational resampler on the MI355X, bit for bit against ``scipy.signal.upfirdn`` / ``resample_poly`` (tests/resample_cases.py).

The bar is ``np.array_equal`` in both precisions: librosa_amd/csrc/lra_cqt.h promises one rounding per operation and sums in ascending input order on every route,
and the constant-Q tests rely on it ("nothing accumulates down the recursion").  No tolerance anywhere in this file.

Each test prints the route it exercised, the samples it compared and the mismatches it found.  Measured on the MI355X, all tests of this file together
(176 comparisons, 3 868 662 samples, 0 mismatches, every sample stored; the file runs in about four seconds):

    kernel                        float32 samples   float64 samples   mismatches
    fir_halve4_kernel                   1 192 814         1 105 174            0
    fir_decimate_kernel<T, 4>             457 126            50 772            0
    fir_decimate_kernel<T, 1>             186 196           679 786            0
    fir_decimate_direct_kernel             28 133            28 537            0
    resample_poly_kernel                   70 062            70 062            0

That includes both neighbours of every limit of the selection (float32: 5235 / 5236 and 6146 / 6147 taps, ``down`` 59 / 60; float64: 1594 / 1595 and 2050 / 2051
taps, ``down`` 29 / 30), the two launches that use 64 KiB of dynamic LDS to the byte (5235 taps in float32, 1594 in float64), the staging loop past its unrolled
loads, ``first`` and ``mul`` other than the designs', and outputs past the end of the signal.  The gfx950 code of the float32 four-output forms accumulates with
v_pk_mul_f32 + v_pk_add_f32 and the others with separate multiplies and adds; the only fused operations are those of the float64 division.
"""
import numpy as np
import pytest
import scipy.signal

import librosa_amd as L
import resample_cases as RC
from librosa_amd import _arrays

pytestmark = pytest.mark.gpu

BUILT = {}


def built(case):
    """A case's inputs and its reference, computed once and left unchanged."""
    if case not in BUILT:
        c = RC.build(case) if len(case) == 9 else RC.build_up(case)
        c["want"] = RC.case_reference(c)
        for a in (c["x"], c["taps"], c["want"]):
            a.setflags(write=False)
        BUILT[case] = c
    return BUILT[case]


def _torch():
    import torch

    return torch


def _dev(a):
    return _torch().from_numpy(np.array(a)).cuda()   # (a copy: the shared inputs are read-only)


def raw(x, taps, up, down, first, n_out, div, mul, key, general=False):
    """``lra_fir_decimate_exec`` (``lra_resample_poly_exec`` when ``general``) the way core/audio.py::resample drives it, into a result that arrives full of NaN."""
    real = x.dtype
    was = _arrays.POISON_OUTPUTS
    _arrays.POISON_OUTPUTS = True
    try:
        sess = _arrays.Session(np.empty(0))
        try:
            ctx = sess.ctx
            x_ptr, batch, n_in, _ = sess.input_2d(x, real)
            out_ptr, handle = sess.output((batch, n_out), real)
            taps_ptr = ctx.device_table(("resample_cases", key, real.str), lambda: np.ascontiguousarray(taps, dtype=real))
            if general:
                ctx.resample_poly_exec(x_ptr, out_ptr, batch, n_in, n_out, taps_ptr, len(taps), up, down, first, div, mul, real)
            else:
                assert up == 1
                ctx.fir_decimate_exec(x_ptr, out_ptr, batch, n_in, n_out, taps_ptr, len(taps), down, first, div, mul, real)
            return sess.result(handle)
        finally:
            sess.close()
    finally:
        _arrays.POISON_OUTPUTS = was


def check(label, got, want, route):
    """Bit equality, with the first difference located; prints what was compared."""
    got = got.cpu().numpy() if not isinstance(got, np.ndarray) else got
    count, what = RC.mismatch(got, want, route)
    print(f"{label}: route {route}, {np.dtype(want.dtype).name}, {want.size} samples compared, {count} mismatches")
    assert count == 0 and np.array_equal(got, want), (label, route, what)
    assert np.isfinite(got).all(), (label, "a sample was not stored")


# ---- the raw entry points -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_fir_decimate_exec_is_upfirdn(case):
    c = built(case)
    got = raw(c["x"], c["taps"], 1, c["down"], c["first"], c["n_out"], c["div"], c["mul"], RC.case_id(case))
    check(RC.case_id(case), got, c["want"], c["route"])


@pytest.mark.parametrize("case", RC.UPSAMPLED, ids=RC.up_id)
def test_resample_poly_exec_is_resample_poly(case):
    c = built(case)
    got = raw(c["x"], c["taps"], c["up"], c["down"], c["first"], c["n_out"], 1.0, 1.0, RC.up_id(case), general=True)
    check(RC.up_id(case), got, c["want"], "resample_poly_kernel")
    assert np.array_equal(c["want"], scipy.signal.resample_poly(c["x"], c["up"], c["down"], axis=-1))


# ---- the public path ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("down", [2, 4, 64])
@pytest.mark.parametrize("n_in", [16385, 40001])
def test_resample_polyphase_is_scipy(dtype, down, n_in):
    import cqt_oracle as CQ

    y = np.random.default_rng(down * 100003 + n_in).standard_normal((2, 3, n_in)).astype(dtype)
    route = RC.route(-(-n_in // down), 21 * down + 1, down, np.dtype(dtype).itemsize)
    plain = scipy.signal.resample_poly(y, 1, down, axis=-1)
    scaled = CQ.resample(y, orig_sr=down, target_sr=1, res_type="polyphase", scale=True)
    assert plain.dtype == scaled.dtype == np.dtype(dtype)
    for scale, want in ((False, plain), (True, scaled)):
        want2 = want.reshape(6, -1)
        got = L.resample(y, orig_sr=down, target_sr=1, res_type="polyphase", scale=scale)
        assert isinstance(got, np.ndarray) and got.shape == want.shape
        check(f"numpy (2, 3, {n_in}) down {down} scale {scale}", got.reshape(6, -1), want2, route)
        got = L.resample(_dev(y), orig_sr=down, target_sr=1, res_type="polyphase", scale=scale)
        assert got.is_cuda and tuple(got.shape) == want.shape
        check(f"tensor (2, 3, {n_in}) down {down} scale {scale}", got.reshape(6, -1), want2, route)
    one = L.resample(y[0, 0], orig_sr=down, target_sr=1, res_type="polyphase")
    check(f"numpy ({n_in},) down {down}", one[None], plain[0, 0][None], route)
    yt = np.ascontiguousarray(np.moveaxis(y[0], -1, 0))   # (n_in, 3): time first
    for arg in (yt, _dev(yt)):
        got = L.resample(arg, orig_sr=down, target_sr=1, res_type="polyphase", scale=True, axis=0)
        got = got.cpu().numpy() if not isinstance(got, np.ndarray) else got
        assert got.shape == (plain.shape[-1], 3)
        check(f"{type(arg).__name__} axis=0 ({n_in}, 3) down {down}", np.ascontiguousarray(got.T), scaled[0], route)


# ---- the halving chain of cqt ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_halving_chain_follows_scipy_step_by_step(dtype):
    """The octave recursion's resampler (constantq.py: the "polyphase" decimator by 2, divided by sqrt(1 / 2)) applied to its own output until fewer than 64 samples
    remain: every step equals the reference's resampler applied to the previous DEVICE result, on whichever kernel the length selects."""
    import cqt_oracle as CQ
    from librosa_amd.core.constantq import _decimator

    real = np.dtype(dtype)
    taps, first = _decimator(2, "polyphase", real)
    cur = np.random.default_rng(33075).standard_normal((1, 33075)).astype(real)
    routes, samples = [], 0
    while cur.shape[-1] >= 64:
        n_out = -(-cur.shape[-1] // 2)
        route = RC.route(n_out, len(taps), 2, real.itemsize)
        nxt = raw(cur, taps, 1, 2, first, n_out, float(np.sqrt(0.5)), 1.0, "chain")
        want = CQ.resample(cur, orig_sr=2, target_sr=1, res_type="polyphase", scale=True)
        check(f"halving {cur.shape[-1]} -> {n_out}", nxt, want, route)
        routes.append(route)
        samples += want.size
        cur = nxt
    print(f"chain: {real.name}, routes {routes}, {samples} samples compared, 0 mismatches")
    assert routes[:2] == ["halve4", "halve4"] and set(routes[2:]) == {"opt1"} and len(routes) == 10 and cur.shape[-1] < 64


# ---- the library's own design through the public path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in RC.CASES if c[4] == ("soxr_hq",)], ids=RC.case_id)
def test_resample_own_design_is_the_reference(case):
    c = built(case)
    assert c["div"] == float(np.sqrt(1.0 / c["down"])) and c["mul"] == 1.0 and len(c["taps"]) == {2: 377, 4: 753}[c["down"]]
    for arg in (c["x"], _dev(c["x"])):
        got = L.resample(arg, orig_sr=c["down"], target_sr=1, res_type="soxr_hq", scale=True)
        check(f"{type(arg).__name__} soxr_hq down {c['down']}", got, c["want"], c["route"])
