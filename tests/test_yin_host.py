"""yin without a GPU: the NumPy model against tests/golden/yin.npz, the certification of the cases, every argument error before any device
work, the exported names, and the kernel bodies of librosa_amd/csrc/lra_yin.h run on host threads (tests/hostsim/yinsim.cpp).

Measured through the simulator (settled frames): f0 within 1.6e-15 relative of the float64 model at worst, against bounds of 8.9e-16 .. 1.2e-14
(16 x the reference's own distance from the exact evaluation, at least 4 ulp); no settled frame at another lag than the reference's; 1 of 1086
live frames is unsettled."""
import ctypes
import os
import warnings

import numpy as np
import pytest

import hostsim_util
import librosa_amd as L
import yin_cases as YC
from librosa_amd.core import pitch as P

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "librosa_amd", "csrc")
PAD_MODES = {"constant": 0, "reflect": 1, "edge": 2, "symmetric": 3}


@pytest.fixture(scope="module")
def golden():
    return YC.load()


model64, settled = YC.model64, YC.settled_frames


# ---- the golden file and the model ----------------------------------------------------------------------------------------------------------
def test_golden_covers_the_cases(golden):
    z, meta = golden
    assert set(meta["cases"]) == set(YC.CASES) and set(meta["errors"]) == set(YC.ERRORS)
    for name in YC.CASES:
        assert meta["cases"][name]["y"] == YC.digest(YC.signal(name)), name
    assert os.path.getsize(YC.GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", list(YC.CASES))
def test_model_matches_the_reference(golden, name):
    z, meta = golden
    y, kw = YC.signal(name), YC.CASES[name]["kw"]
    m = YC.model(y, **kw)
    want = z["f0_" + name]
    assert m["f0"].dtype == want.dtype == np.dtype(meta["cases"][name]["f0_dtype"]) and m["f0"].shape == want.shape and want.size == meta["cases"][name]["frames"]
    assert np.max(YC.rel_err(m["f0"], want), initial=0) <= 1e-12
    cm = z["cmnd_" + name]
    assert cm.dtype == y.dtype and cm.shape == m["cmnd"].shape
    np.testing.assert_allclose(m["cmnd"].astype(y.dtype), cm, rtol=4 * np.finfo(y.dtype).eps, atol=4 * np.finfo(y.dtype).eps)
    if m["silent"].any():
        assert np.all(want[m["silent"]] == kw["sr"] / m["min_period"])  # exact


def test_cases_are_certified(golden):
    z, meta = golden
    live = bad = 0
    for name in YC.CASES:
        m = model64(name)
        ok = settled(name, meta)
        n_live = int((~m["silent"]).sum())
        n_bad = n_live - int(ok.sum())
        assert n_bad <= YC.MAX_UNSETTLED_CASE * n_live, (name, n_bad, n_live)
        assert n_bad == meta["cases"][name]["unsettled"], name
        # on settled frames the reference chose the model's lag
        want = z["f0_" + name]
        lag = YC.CASES[name]["kw"]["sr"] / want[ok] - m["min_period"]
        assert np.all(np.abs(lag - (m["index"][ok] + np.take_along_axis(m["shifts"], m["index"][..., None, :], axis=-2)[..., 0, :][ok])) < 1e-3), name
        live += n_live
        bad += n_bad
    assert bad <= YC.MAX_UNSETTLED_ALL * live, (bad, live)


def test_case_families_are_present(golden):
    _, meta = golden
    c = meta["cases"]
    assert c["w512_zeros"]["silent"] == c["w512_zeros"]["frames"] > 0
    assert all(c[n]["silent"] > 0 for n in ("w512_gap", "w512_gap64", "w1001_gap64"))
    assert c["first_lag"]["lags"] == [0, 0] and c["last_lag"]["lags"] == [c["last_lag"]["n_lags"] - 1] * 2
    assert [c[f"frames{n}"]["frames"] for n in (1, 15, 16, 17)] == [1, YC.FRAME_RUN - 1, YC.FRAME_RUN, YC.FRAME_RUN + 1]
    assert YC.periods(YC.CASES["nyquist"]["kw"])[0] == 2 and c["w64_glide"]["n_lags"] == 27
    assert c["two_periods_warning"]["warned"] and "less than two periods" in c["two_periods_warning"]["warned"][0]
    assert {YC.CASES[n]["kw"].get("trough_threshold", 0.1) for n in YC.CASES} >= {0.0, 0.1, 1.0}
    assert {YC.CASES[n]["lead"] for n in YC.CASES} >= {(), (2,), (2, 3)} and {YC.CASES[n]["dtype"] for n in YC.CASES} == {"float32", "float64"}


# ---- argument errors: raised before any device call (this host has no GPU: a device call would raise NativeError) ---------------------------
@pytest.mark.parametrize("name", list(YC.ERRORS))
def test_argument_errors_match_the_reference(golden, name):
    _, meta = golden
    y, kw = YC.error_call(name)
    want = meta["errors"][name]
    assert want["type"] == "ParameterError"
    with pytest.raises(L.ParameterError) as info:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            L.yin(y, **kw)
    assert str(info.value) == want["message"]
    if name not in ("no_fmin", "no_fmax"):
        with pytest.raises(L.ParameterError):
            P._yin_frames(y, **kw)


def test_two_period_warning_comes_before_device_work(golden):
    _, meta = golden
    kw = YC.CASES["two_periods_warning"]["kw"]
    with pytest.warns(UserWarning) as seen:
        with pytest.raises(L.ParameterError):  # the warning is issued by the parameter check; the too-short signal stops the call right after
            L.yin(np.ones(10, np.float32), center=False, **kw)
    assert str(seen[0].message) == meta["cases"]["two_periods_warning"]["warned"][0]


def test_bounds_are_keyword_only_and_required():
    with pytest.raises(TypeError):
        L.yin(np.ones(4096, np.float32))
    with pytest.raises(TypeError):
        L.yin(np.ones(4096, np.float32), 100.0, 2000.0)


def test_names_are_exported():
    assert L.yin is L.core.yin is P.yin
    assert "yin" in L.__all__ and "yin" in L.core.__all__ and "yin" in P.__all__
    assert callable(P._yin_frames)
    from librosa_amd import _native

    assert "lra_yin_exec" in _native.SIGNATURES and (_native.Context.YIN_F0, _native.Context.YIN_FRAMES) == (P._YIN_F0, P._YIN_FRAMES) == (0, 1)


# ---- the kernel bodies on host threads ------------------------------------------------------------------------------------------------------
_sim = None


def sim_lib():
    global _sim
    if _sim is None:
        _sim = hostsim_util.sim_lib("yinsim", pthread=True)
        c = ctypes
        _sim.yinsim_exec.argtypes = [c.c_void_p, c.c_longlong, c.c_longlong, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_double, c.c_double, c.c_int, c.c_void_p,
                                     c.c_void_p, c.c_void_p, c.c_int]
        _sim.yinsim_geometry.argtypes = [c.c_int, c.c_int, c.c_void_p]
    return _sim


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def geometry(W, P_):
    out = np.zeros(4, np.int32)
    sim_lib().yinsim_geometry(int(W), int(P_), _p(out))
    return dict(run=int(out[0]), N=int(out[1]), chunk=int(out[2]), lds=int(out[3]))


def sim_exec(y, mode, *, fmin, fmax, sr=YC.SR, frame_length=2048, hop_length=None, trough_threshold=0.1, center=True, pad_mode="constant", direct=False):
    """One lra_yin_exec through the simulator, prepared as librosa_amd.yin prepares it; the outputs arrive full of NaN: every element must be stored."""
    y, real, hop, center, pad_mode, p0, p1 = P._yin_prepare(y, fmin, fmax, sr, frame_length, hop_length, center, pad_mode)
    y = np.ascontiguousarray(y, dtype=real)
    before = y.copy()
    lead, n = y.shape[:-1], y.shape[-1]
    batch = int(np.prod(lead)) if lead else 1
    nf = 1 + (n + (2 * (frame_length // 2) if center else 0) - frame_length) // hop
    f0 = np.full((batch, nf), np.nan)
    frames = np.full((2, batch, p1 - p0 + 1, nf), np.nan, dtype=real)
    rc = sim_lib().yinsim_exec(_p(y), batch, n, int(real == np.float64), frame_length, hop, int(center), PAD_MODES[pad_mode], p0, p1, float(trough_threshold), float(sr), mode,
                               _p(f0), _p(frames[0]), _p(frames[1]), int(direct))
    assert rc == 0
    assert np.array_equal(y, before), "the input was written"
    if mode == P._YIN_F0:
        assert not np.isnan(f0).any()
        return f0.reshape(lead + (nf,))
    assert not np.isnan(frames).any()
    return frames[0].reshape(lead + frames.shape[2:]), frames[1].reshape(lead + frames.shape[2:])


def test_case_geometry_matches_the_kernels_constants():
    assert geometry(64, 28)["run"] == YC.FRAME_RUN
    want = {"w64_glide": 160, "w512_glide": 800, "w1001_glide": 1280, "w2048_glide": 2400, "w4500_glide": 0, "two_periods_warning": 882}
    chunks = set()
    for name, N in want.items():
        kw = YC.CASES[name]["kw"]
        p0, p1 = YC.periods(kw)
        g = geometry(kw["frame_length"], p1)
        assert g["N"] == N == YC.transform_length(kw["frame_length"], p1), name
        assert g["chunk"] == (YC.chunk_frames(N) if N else 1) and g["lds"] <= 160 * 1024, name
        chunks.add(g["chunk"])
    assert chunks >= {1, 2, 16}  # whole run at once, part chunks, one frame at a time
    assert 2400 < 4096  # the reference pads the default frame to 4096 points
    # the direct-path switch: the largest compiled size is the last that a transform serves
    assert geometry(4800 - 340, 340)["N"] == 4800 and geometry(4800 - 339, 340)["N"] == 0
    # the direct kernel's two rows of lags: 10239 lags are the last that fit a workgroup's 160 KiB
    assert geometry(8192, 8191)["lds"] <= 160 * 1024 and geometry(16384, 10239)["lds"] <= 160 * 1024 < geometry(16384, 10240)["lds"]
    # the cases that have to ask for more than 64 KiB
    for name, N in (("w2048_fmin11", 4800), ("w8192_fmin5", 0)):
        kw = YC.CASES[name]["kw"]
        g = geometry(kw["frame_length"], YC.periods(kw)[1])
        assert g["N"] == N and 64 * 1024 < g["lds"] <= 160 * 1024, (name, g)


def test_size_lists_are_the_librarys():
    """tests/yin_cases.py carries a copy of LRA_MIXED_SIZES: it must be csrc/lra_mixed_sizes.h's list, which the simulators include and nothing
    repeats; and the simulator's choice of transform must be the library's own (lra_yin_lds_bytes: host arithmetic on the library's list, no device)."""
    import glob
    import re

    from librosa_amd import _native

    text = open(os.path.join(CSRC, "lra_mixed_sizes.h")).read()
    line = re.search(r"#define LRA_MIXED_SIZES\(X\)(.*)", text).group(1)
    sizes = tuple(int(v) for v in re.findall(r"X\((\d+)\)", line))
    assert sizes == YC.SIZES and len(sizes) >= 25
    sources = glob.glob(os.path.join(CSRC, "*")) + glob.glob(os.path.join(HERE, "hostsim", "*.cpp")) + glob.glob(os.path.join(HERE, "hostsim", "*.h"))
    assert sum(open(f, errors="replace").read().count("#define LRA_MIXED_SIZES") for f in sources if os.path.isfile(f)) == 1
    lib = _native.load_library()
    for N in sizes + (4801,):  # at, one below and one above every size: where the choice changes
        for total in (N - 1, N, N + 1):
            P_ = min(27, total // 3)
            W = total - P_
            g = geometry(W, P_)
            assert g["N"] == YC.transform_length(W, P_), (W, P_)
            assert g["lds"] == lib.lra_yin_lds_bytes(W, P_), (W, P_)


def test_a_period_range_beyond_the_lds_is_refused_before_device_work():
    y = np.zeros(40000, np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (less than two periods fit: the reference's warning comes first)
        with pytest.raises(L.ParameterError, match="max_period=11025"):
            L.yin(y, fmin=4.0, fmax=2000.0, sr=44100, frame_length=16384)
        with pytest.raises(L.ParameterError, match="max_period=11025"):
            P._yin_frames(y, fmin=4.0, fmax=2000.0, sr=44100, frame_length=16384)


SIM_CASES = [n for n in YC.CASES]


@pytest.mark.parametrize("name", SIM_CASES)
def test_simulated_f0_matches_the_model_and_the_reference(golden, name):
    z, meta = golden
    y, kw = YC.signal(name), YC.CASES[name]["kw"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = sim_exec(y, P._YIN_F0, **kw)
    YC.check_f0(got, name, z, meta)


@pytest.mark.parametrize("name", ["w64_glide", "w512_gap", "w512_glide64", "w1001_gap64", "w2048_glide", "w4500_gap64", "lead2", "nocenter", "reflect", "nyquist", "last_lag", "two_periods_warning"])
def test_simulated_frames_match_the_reference(golden, name):
    z, meta = golden
    y, kw = YC.signal(name), dict(YC.CASES[name]["kw"])
    kw.pop("trough_threshold", None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cm, sh = sim_exec(y, P._YIN_FRAMES, **kw)
    m = model64(name)
    want = z["cmnd_" + name]
    assert cm.dtype == sh.dtype == y.dtype and cm.shape == sh.shape == want.shape
    YC.check_frames(cm, sh, m, want, meta["cases"][name], y.dtype)


def test_direct_kernel_matches_the_transform():
    for name in ("w64_noise64", "w512_gap", "frames17"):
        y, kw = YC.signal(name), YC.CASES[name]["kw"]
        a = sim_exec(y, P._YIN_F0, **kw)
        b = sim_exec(y, P._YIN_F0, direct=True, **kw)
        m = model64(name)
        ok = YC.settled(m["cmnd"], kw.get("trough_threshold", 0.1), 1e-9) & ~m["silent"]
        assert ok.mean() > 0.5 and np.max(YC.rel_err(b[ok], a[ok])) <= 1e-13
        assert np.array_equal(a[m["silent"]], b[m["silent"]])


def test_a_clip_gives_the_same_bits_alone_and_in_a_batch():
    y, kw = YC.signal("lead2"), YC.CASES["lead2"]["kw"]
    whole = sim_exec(y, P._YIN_F0, **kw)
    one = sim_exec(y[1, 2], P._YIN_F0, **kw)
    assert np.array_equal(whole[1, 2], one)
