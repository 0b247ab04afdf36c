"""The cases of tests/test_resample_host.py and tests/test_resample_gpu.py: every route of ``lra_fir_decimate_exec`` (librosa_amd/csrc/lra_api.hip) and the
general rational resampler of ``lra_resample_poly_exec``, against ``scipy.signal.upfirdn`` -- the plain C loop whose summation order the kernels of
librosa_amd/csrc/lra_cqt.h promise to reproduce bit for bit.  Every input is seeded and every expectation is computed: there is no fixture file.

``route()`` restates the selection of ``lra_fir_decimate_exec``; it is the second copy of it (the first is ``fir_plan`` of librosa_amd/csrc/lra_cqt.h, which
the library launches from and the host simulator runs; the host test compares that one with this one)."""
import numpy as np
import scipy.signal

ROUTES = ("halve4", "opt4", "opt1", "direct")   # fir_halve4_kernel, fir_decimate_kernel<T, 4>, fir_decimate_kernel<T, 1>, fir_decimate_direct_kernel


def route(n_out, n_taps, down, elem):
    """The kernel ``lra_fir_decimate_exec`` launches for ``n_out`` outputs per clip, ``n_taps`` taps, decimation ``down`` and ``elem`` bytes per sample."""
    four = n_out >= 8192 and (1023 * down + n_taps) * elem <= 32 * 1024
    span2 = 1023 * 2 + n_taps
    lds2 = (span2 + span2 // 8 + 1) * 2 * elem
    if four and down == 2 and lds2 <= 64 * 1024:
        return "halve4"
    if four:
        return "opt4"
    if (255 * down + n_taps) * elem <= 64 * 1024:
        return "opt1"
    return "direct"


def reference(x, taps, up, down, first, n_out, div=1.0, mul=1.0):
    """``x``: (batch, n_in) -> (batch, n_out): scipy's upfirdn, outputs ``first .. first + n_out - 1`` (zeros past its end), then the two roundings the kernels
    apply: ``(T)((double)v / div)`` and, when ``mul != 1``, ``(T)((double)that * mul)``."""
    x = np.ascontiguousarray(x)
    taps = np.ascontiguousarray(taps, dtype=x.dtype)
    full = scipy.signal.upfirdn(taps, x, up, down, axis=-1)
    assert full.dtype == x.dtype
    kept = full[..., first : first + n_out]
    out = np.zeros(x.shape[:-1] + (n_out,), dtype=x.dtype)
    out[..., : kept.shape[-1]] = kept
    out = (out.astype(np.float64) / np.float64(div)).astype(x.dtype)
    if mul != 1:
        out = (out.astype(np.float64) * np.float64(mul)).astype(x.dtype)
    return out


_HALF, _TWO = float(np.sqrt(0.5)), float(np.sqrt(2.0))
_F = (np.float32, np.float64)

# (dtype, down, n_in, n_out, taps_spec, first, div, mul, batch); first None: the design's own alignment; n_out None: ceil(n_in / down)
CASES = []
for _t in _F:
    # scipy's Kaiser design (21 down + 1 taps with its zero prefix), the scale=True divisor of the octave recursion except where div = 1 is the case
    for _down, _n, _div in ((2, 16385, None), (3, 24577, 1.0), (4, 32769, None), (8, 70000, None), (64, 20000, None), (2, 8191 * 2, 1.0),
                            (29, 4000, None), (30, 4000, None), (59, 4000, None), (60, 4000, None)):   # the last four: either side of the first `down` that goes direct, per precision
        CASES.append((_t, _down, _n, None, ("polyphase",), None, float(np.sqrt(1.0 / _down)) if _div is None else _div, 1.0, 2))
    # the library's own design (377 and 753 taps)
    CASES.append((_t, 2, 20001, None, ("soxr_hq",), None, _HALF, 1.0, 3))
    CASES.append((_t, 4, 33000, None, ("soxr_hq",), None, float(np.sqrt(0.25)), 1.0, 2))
    # random taps, halving: the tail loop alone (7), n_taps % 8 of 0 and 7 beside the unrolled blocks, the staging loop past its ten unrolled loads (515), and the
    # two neighbours of every limit of the table in either precision (lds2: 1594 / 1595 in float64, 5235 / 5236 in float32; 32 KiB: 2050 / 2051 and 6146 / 6147)
    for _n, _taps, _first, _nout in ((16400, 7, 0, 8200), (16400, 64, 5, 8200), (16400, 79, 1, 8195), (16400, 515, 100, 8192), (17000, 1594, 3, 9000), (17000, 1595, 3, 9000),
                                     (17000, 2050, 0, 8193), (17000, 2051, 0, 8193), (18000, 5234, 7, 9217), (18000, 5235, 7, 9217), (18000, 5236, 7, 9217),
                                     (18000, 6146, 0, 8193), (18000, 6147, 0, 8193)):
        CASES.append((_t, 2, _n, _nout, ("random", _taps), _first, _HALF, _TWO, 2))
    CASES.append((_t, 2, 3000, 8192, ("random", 41), 10, _HALF, _TWO, 2))      # outputs from 1510 on lie beyond the signal; blocks 2 .. 7 are fully outside it
    CASES.append((_t, 5, 50000, 10001, ("random", 200), 2, _HALF, _TWO, 3))
CASES = tuple(CASES)

# (dtype, up, down, n): resample_poly_kernel with scipy's design
UPSAMPLED = tuple((_t, _u, _d, _n) for _t in _F for _u, _d, _n in ((3, 2, 9001), (2, 3, 9001), (160, 441, 20000), (441, 160, 3000), (5, 4, 1)))


def case_id(case):
    dtype, down, n_in, n_out, spec, first, div, mul, batch = case
    return f"{np.dtype(dtype).name}-d{down}-n{n_in}-{'-'.join(str(s) for s in spec)}" + ("" if n_out is None else f"-out{n_out}")


def up_id(case):
    dtype, up, down, n = case
    return f"{np.dtype(dtype).name}-{up}over{down}-n{n}"


def _seed(case, table):
    return 20240 + table.index(case)


def build(case):
    """A case of ``CASES`` -> dict(x, taps, down, first, n_out, div, mul, route): the seeded signal, the taps, and the resolved defaults."""
    from librosa_amd.core.constantq import _decimator

    dtype, down, n_in, n_out, spec, first, div, mul, batch = case
    real = np.dtype(dtype)
    rng = np.random.default_rng(_seed(case, CASES))
    x = rng.standard_normal((batch, n_in)).astype(real)
    if spec[0] == "random":
        taps = rng.standard_normal(spec[1]).astype(real)
        assert first is not None and n_out is not None
    else:
        taps, own_first = _decimator(down, spec[0], real)
        first = own_first if first is None else first
    n_out = -(-n_in // down) if n_out is None else n_out
    return dict(x=x, taps=np.ascontiguousarray(taps), down=down, first=int(first), n_out=int(n_out), div=div, mul=mul, route=route(n_out, len(taps), down, real.itemsize))


def build_up(case):
    """A case of ``UPSAMPLED`` -> dict(x, taps, up, down, first, n_out)."""
    from librosa_amd.core.audio import _rational_filter

    dtype, up, down, n = case
    real = np.dtype(dtype)
    x = np.random.default_rng(_seed(case, UPSAMPLED)).standard_normal((2, n)).astype(real)
    taps, first = _rational_filter(up, down, "polyphase", real)
    return dict(x=x, taps=np.ascontiguousarray(taps), up=up, down=down, first=int(first), n_out=-(-n * up // down))


def case_reference(c):
    """``reference()`` of a built case (either table)."""
    return reference(c["x"], c["taps"], c.get("up", 1), c["down"], c["first"], c["n_out"], c.get("div", 1.0), c.get("mul", 1.0))


def ulps(a, b):
    """Distance of two scalars of one precision in units in the last place of the larger (inf when either is not finite)."""
    if not (np.isfinite(a) and np.isfinite(b)):
        return float("inf")
    return float(abs(np.float64(a) - np.float64(b)) / np.spacing(max(abs(a), abs(b), np.finfo(type(a)).tiny)))


def mismatch(got, want, route_name=None):
    """(count of differing samples, description of the first: its clip and index, the block of outputs it belongs to, the difference in ulps) -- a failure then
    points at staging (a whole block, or its edges), the tap tail (every sample, small) or rounding (scattered, 1 ulp)."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return max(got.size, want.size), f"shape / dtype {got.shape} {got.dtype}, expected {want.shape} {want.dtype}"
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    count = int(bad.sum())
    if not count:
        return 0, ""
    clip, idx = (int(v) for v in np.argwhere(bad)[0])
    per_block = {"halve4": 1024, "opt4": 1024, "opt1": 256, "direct": 256}.get(route_name, 256)
    g, w = got[clip, idx], want[clip, idx]
    return count, (f"{count} of {got.size} samples differ; first at clip {clip} index {idx} (block {idx // per_block} of {per_block} outputs, offset {idx % per_block}): "
                   f"got {g!r}, expected {w!r}, {ulps(g, w):.3g} ulp; {int(np.isnan(got).sum())} samples not stored")
