"""The FIR decimator routes and the rational resampler without a GPU: that tests/resample_cases.py reaches every kernel of ``lra_fir_decimate_exec`` on either
side of every limit of its selection, that the kernel bodies of librosa_amd/csrc/lra_cqt.h run on host threads (tests/hostsim/postsim.cpp) equal
``scipy.signal.upfirdn`` bit for bit on every case, that the reference restatement is scipy's entry point, and that the library's own selection (``fir_plan`` of lra_cqt.h, which the simulator runs
and exports) is ``resample_cases.route()``."""
import numpy as np
import pytest
import scipy.signal

import hostsim_util as H
import resample_cases as RC

BUILT = {}


def built(case):
    """A case's inputs and its reference, computed once."""
    if case not in BUILT:
        c = RC.build(case) if len(case) == 9 else RC.build_up(case)
        c["want"] = RC.case_reference(c)
        c["want"].setflags(write=False)
        BUILT[case] = c
    return BUILT[case]


# ---- route coverage -------------------------------------------------------------------------------------------------------------------------
def _routes(elem):
    return [built(c)["route"] for c in RC.CASES if np.dtype(c[0]).itemsize == elem]


@pytest.mark.parametrize("elem", [4, 8])
def test_cases_take_every_route(elem):
    routes = _routes(elem)
    assert set(routes) == set(RC.ROUTES), {r: routes.count(r) for r in RC.ROUTES}
    print({r: routes.count(r) for r in RC.ROUTES})


def _has(elem, pred):
    return any(np.dtype(c[0]).itemsize == elem and pred(built(c)) for c in RC.CASES)


@pytest.mark.parametrize("elem", [4, 8])
def test_cases_lie_on_either_side_of_every_inequality(elem):
    """Every condition of the selection, true in one case and false in another, everything before it in the table being equal."""
    n_taps = lambda c: len(c["taps"])  # noqa: E731
    fits32 = lambda c: (1023 * c["down"] + n_taps(c)) * elem <= 32 * 1024  # noqa: E731
    lds2 = lambda c: (2046 + n_taps(c) + (2046 + n_taps(c)) // 8 + 1) * 2 * elem  # noqa: E731
    fits64 = lambda c: (255 * c["down"] + n_taps(c)) * elem <= 64 * 1024  # noqa: E731
    # n_out >= 8192 (with a span that fits): 8191 against 8192 and 8193
    assert _has(elem, lambda c: c["n_out"] == 8191 and fits32(c) and c["route"] == "opt1")
    assert _has(elem, lambda c: c["n_out"] == 8192 and c["route"] == "halve4") and _has(elem, lambda c: c["n_out"] == 8193 and c["route"] == "halve4")
    # the 32 KiB span, big jobs only
    assert _has(elem, lambda c: c["n_out"] >= 8192 and fits32(c)) and _has(elem, lambda c: c["n_out"] >= 8192 and not fits32(c) and c["route"] == "opt1")
    # down == 2, four outputs per thread either way
    assert _has(elem, lambda c: c["route"] == "opt4" and c["down"] != 2) and _has(elem, lambda c: c["route"] == "opt4" and c["down"] == 2 and lds2(c) > 64 * 1024)
    # lds2 against 64 KiB: the last size that fits is used to the byte
    assert _has(elem, lambda c: c["route"] == "halve4" and lds2(c) == 64 * 1024) and _has(elem, lambda c: c["route"] == "opt4" and 64 * 1024 < lds2(c) <= 64 * 1024 + 2 * 2 * elem)
    # the 64 KiB span of the one-output form
    assert _has(elem, lambda c: c["route"] == "opt1" and fits64(c)) and _has(elem, lambda c: c["route"] == "direct" and not fits64(c))


# (elem, what changes, the two neighbours, their routes): n_taps at down == 2 and 9000 outputs, or `down` with scipy's 21 down + 1 taps and 100 outputs
BOUNDARIES = [
    (4, "n_taps", (5235, 5236), ("halve4", "opt4")),    # lds2: (2046 + 5235) * 9 // 8 + 1 = 8192 pairs of 8 bytes are 64 KiB to the byte (5234 is inside, 8191 pairs)
    (8, "n_taps", (1594, 1595), ("halve4", "opt4")),    # lds2: 4096 pairs of 16 bytes
    (4, "n_taps", (6146, 6147), ("opt4", "opt1")),      # 32 KiB: 2046 + 6146 = 8192 floats
    (8, "n_taps", (2050, 2051), ("opt4", "opt1")),      # 32 KiB: 2046 + 2050 = 4096 doubles
    (4, "down", (59, 60), ("opt1", "direct")),          # 64 KiB: 276 down + 1 samples
    (8, "down", (29, 30), ("opt1", "direct")),
]


@pytest.mark.parametrize("elem,what,pair,routes", BOUNDARIES)
def test_route_boundaries(elem, what, pair, routes):
    for v, r in zip(pair, routes):
        got = RC.route(9000, v, 2, elem) if what == "n_taps" else RC.route(100, 21 * v + 1, v, elem)
        assert got == r, (elem, what, v, got)
    if what == "n_taps":   # both neighbours are cases, and run where this says
        for v, r in zip(pair, routes):
            assert _has(elem, lambda c: c["down"] == 2 and len(c["taps"]) == v and c["n_out"] >= 8192 and c["route"] == r), (elem, v)
    else:
        from librosa_amd.core.constantq import _decimator

        real = np.dtype(np.float32 if elem == 4 else np.float64)
        for v, r in zip(pair, routes):
            assert len(_decimator(v, "polyphase", real)[0]) == 21 * v + 1
            assert _has(elem, lambda c: c["down"] == v and c["route"] == r), (elem, v)


def test_float32_lds2_limit_is_one_tap_later_than_5234():
    """5234 and 5235 taps both still take the halving kernel in float32 (8191 and 8192 staged pairs); both stay cases, beside 5236."""
    assert [RC.route(9000, t, 2, 4) for t in (5234, 5235, 5236)] == ["halve4", "halve4", "opt4"]


def test_halving_kernel_stays_inside_its_lds():
    """fir_halve4_kernel's highest staged slot and highest slot read, against the pairs ``lds2`` pays for, for every filter length it can be launched with
    (the simulator's LDS is larger than any launch's, so it would not notice)."""
    for elem, longest in ((4, 5235), (8, 1594)):
        assert RC.route(9000, longest, 2, elem) == "halve4" and RC.route(9000, longest + 1, 2, elem) != "halve4"
        n_taps = np.arange(1, longest + 1)
        span2 = 2046 + n_taps
        pairs = span2 + span2 // 8 + 1
        assert np.all(pairs * 2 * elem <= 64 * 1024)
        staged_top = (span2 - 1) + (span2 - 1) // 8              # put(span2 - 1, ...)
        j_top = n_taps + 3                                        # pair_at(k + u + 4), k + 8 <= n_taps, u <= 7; pair_at(k + 4), k < n_taps
        read_top = 255 * 9 + j_top + j_top // 8
        assert np.all(staged_top < pairs) and np.all(read_top < pairs)
        assert np.all(255 * 8 + j_top + 2 <= span2 - 1)           # the second half of the last pair read is a staged sample


# ---- the simulator against the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_fir_decimate_body_is_upfirdn(case):
    c = built(case)
    got = H.fir_decimate(c["x"], c["taps"], c["down"], c["first"], c["n_out"], div=c["div"], mul=c["mul"])   # (arrives full of NaN: every sample is stored)
    count, what = RC.mismatch(got, c["want"], c["route"])
    assert count == 0 and np.array_equal(got, c["want"]), (RC.case_id(case), c["route"], what)
    assert np.isfinite(got).all() and np.abs(c["want"]).max() > 0


@pytest.mark.parametrize("case", RC.UPSAMPLED, ids=RC.up_id)
def test_resample_poly_body_is_upfirdn_and_resample_poly(case):
    c = built(case)
    got = H.resample_poly(c["x"], c["taps"], c["up"], c["down"], c["first"], c["n_out"])
    count, what = RC.mismatch(got, c["want"])
    assert count == 0 and np.array_equal(got, c["want"]), (RC.up_id(case), what)
    want = scipy.signal.resample_poly(c["x"], c["up"], c["down"], axis=-1)
    assert want.dtype == got.dtype and np.array_equal(c["want"], want)


# ---- the reference restatement is scipy's entry point ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in RC.CASES if c[4] == ("polyphase",) and c[5] is None], ids=RC.case_id)
def test_reference_is_scipy_resample_poly(case):
    c = built(case)
    plain = RC.reference(c["x"], c["taps"], 1, c["down"], c["first"], c["n_out"])
    want = scipy.signal.resample_poly(c["x"], 1, c["down"], axis=-1)
    assert plain.dtype == want.dtype and np.array_equal(plain, want)
    if c["div"] != 1.0:   # the scale=True form of librosa.resample, as the oracle restates it
        import cqt_oracle as CQ

        assert np.array_equal(c["want"], CQ.resample(c["x"], orig_sr=c["down"], target_sr=1, res_type="polyphase", scale=True))


# ---- the library's own selection (lra_cqt.h: fir_plan, what lra_fir_decimate_exec launches and the simulator runs) against route() ------------
def test_plan_geometry_is_what_the_route_implies():
    """blocks_per_clip and lds_bytes of every case, from route()'s arithmetic: 1024 outputs a workgroup on the four-output routes and 256 on the others; the padded
    span of pairs for the halving kernel, the workgroup's input span for the strided ones, nothing for the direct one.  No staged route asks for more than 64 KiB."""
    for case in RC.CASES:
        c = built(case)
        elem, n_taps, down, n_out = c["x"].dtype.itemsize, len(c["taps"]), c["down"], c["n_out"]
        plan = H.fir_plan(n_out, n_taps, down, elem == 8)
        opt = 4 if c["route"] in ("halve4", "opt4") else 1
        span2 = 2046 + n_taps
        lds = {"halve4": (span2 + span2 // 8 + 1) * 2 * elem, "opt4": (1023 * down + n_taps) * elem, "opt1": (255 * down + n_taps) * elem, "direct": 0}[c["route"]]
        assert plan == dict(route=c["route"], opt=opt, blocks_per_clip=-(-n_out // (256 * opt)), lds_bytes=lds), RC.case_id(case)
        assert plan["lds_bytes"] <= 64 * 1024 and (plan["lds_bytes"] > 0) == (c["route"] != "direct"), RC.case_id(case)


def test_simulator_routes_like_route():
    for case in RC.CASES:
        c = built(case)
        assert H.fir_route(c["n_out"], len(c["taps"]), c["down"], c["x"].dtype == np.float64) == c["route"], RC.case_id(case)
    for elem in (4, 8):   # and around every limit, cases or not
        for n_out in (1, 8191, 8192, 20000):
            for down in (1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 29, 30, 31, 32, 59, 60, 64, 128, 300):
                for n_taps in (1, 43, 377, 1594, 1595, 2050, 2051, 4000, 5234, 5235, 5236, 6146, 6147, 8191, 8192, 8193, 16384, 16385, 70000):
                    assert H.fir_route(n_out, n_taps, down, elem == 8) == RC.route(n_out, n_taps, down, elem), (elem, n_out, down, n_taps)
