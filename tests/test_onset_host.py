"""onset_strength / onset_strength_multi without a GPU: argument checks before any device work, the golden fixture, and the kernel bodies of
librosa_amd/csrc/lra_onset.h run on host threads (tests/hostsim/onsetsim.cpp) against the reference's envelopes in tests/golden/onset.npz."""
import ctypes
import json
import os

import numpy as np
import pytest

import hostsim_util
import librosa_amd as L
from librosa_amd import onset as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "onset.npz")

CASE_NAMES = ["default", "lag2_max3", "hop441", "mixed400", "median_channels", "max_slices", "agg_false", "sum", "min", "detrend", "nocenter", "f64", "median_f64_max3", "S_given_ref",
              "S_lag_ge_frames", "S_lag_ge_frames_nocenter", "S_channels_odd", "S_nan_mean", "S_nan_median", "S_nan_max", "S_nan_false", "p75", "feature_amp_mel"]


def p75(x, axis):
    """The custom aggregate of the fixture's "p75" case (scripts/make_onset_golden.py)."""
    return np.percentile(x, 75, axis=axis)


AGGREGATES = dict(mean=np.mean, sum=np.sum, max=np.max, min=np.min, median=np.median, false=False, p75=p75)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


# ---- argument checks: ParameterError before any device call (this host has no GPU: a device call would raise NativeError) ----------------
@pytest.mark.parametrize("kw", [dict(lag=0), dict(lag=1.5), dict(lag=-2), dict(max_size=0), dict(max_size=2.0)])
def test_lag_and_max_size_must_be_positive_integers(kw):
    y = np.zeros(4096, np.float32)
    with pytest.raises(L.ParameterError):
        L.onset.onset_strength(y=y, **kw)
    with pytest.raises(L.ParameterError):
        L.onset.onset_strength_multi(S=np.zeros((8, 10), np.float32), **kw)


def test_aggregate_false_is_rejected_for_the_full_spectrum():
    with pytest.raises(L.ParameterError):
        L.onset.onset_strength(y=np.zeros(4096, np.float32), aggregate=False)


def test_ref_shape_must_match_S():
    S = np.zeros((8, 10), np.float32)
    with pytest.raises(L.ParameterError):
        L.onset.onset_strength_multi(S=S, ref=np.zeros((8, 9), np.float32))
    # the y path: the (always centred) mel's shape is known before the mel is computed
    with pytest.raises(L.ParameterError):
        L.onset.onset_strength(y=np.zeros(4096, np.float32), ref=np.zeros((128, 8), np.float32))
    with pytest.raises(L.ParameterError):
        L.onset.onset_strength(y=np.zeros(4096, np.float32), n_mels=16, ref=np.zeros((16, 9, 1), np.float32))


def test_no_input_is_rejected():
    with pytest.raises(L.ParameterError):
        L.onset.onset_strength()
    with pytest.raises(L.ParameterError):
        L.onset.onset_strength_multi(channels=[0, 4])


def test_bad_channel_sets_are_rejected():
    with pytest.raises(L.ParameterError):
        L.onset.onset_strength_multi(S=np.zeros((8, 10), np.float32), channels=[0, 2.5, 4])
    with pytest.raises(L.ParameterError):
        L.onset.onset_strength_multi(S=np.zeros((8, 10), np.float32), channels=[-1, 4])
    with pytest.raises(ValueError):  # np.max of an empty channel
        L.onset.onset_strength_multi(S=np.zeros((8, 10), np.float32), channels=[slice(3, 3)], aggregate=np.max)


def test_channel_boundaries_follow_util_sync():
    # pad=False for a list of ints: duplicates merge, out-of-range boundaries drop (util.index_to_slice / fix_frames)
    assert O._channel_slices([1, 3, 3, 9], 10) == [slice(1, 3), slice(3, 9)]
    assert O._channel_slices([0, 32, 64, 96, 128], 128) == [slice(0, 32), slice(32, 64), slice(64, 96), slice(96, 128)]
    assert O._channel_slices([2, 200], 128) == []
    assert O._channel_slices(None, 128) == [slice(None)]
    off, idx, widest = O._channel_tables([slice(0, 3), slice(2, 5), slice(None, None, -2)], 6, O._MEAN)
    assert off.tolist() == [0, 3, 6, 9] and idx.tolist() == [0, 1, 2, 2, 3, 4, 5, 3, 1] and widest == 3


# ---- the fixture --------------------------------------------------------------------------------------------------------------------------
def test_golden_fixture_holds_every_case(golden):
    cases = json.loads(str(golden["cases"]))
    assert sorted(cases) == sorted(CASE_NAMES)
    for name in CASE_NAMES:
        assert name in golden.files
        mel = cases[name]["mel"]
        if mel is not None:
            assert f"mel_{mel}" in golden.files and f"db_{mel}" in golden.files
    params = json.loads(str(golden["params"]))
    assert {"numpy", "scipy", "reference_version"} <= set(params)
    assert golden["detrend"].dtype == np.float64 and golden["default"].dtype == np.float32 and golden["f64"].dtype == np.float64
    assert golden["default"].shape == golden["y"].shape[:-1] + (golden["mel_default"].shape[-1],)
    assert os.path.getsize(GOLDEN) < 1 << 20


# ---- the kernel bodies on host threads ------------------------------------------------------------------------------------------------------
_sim = None


def sim_lib():
    global _sim
    if _sim is None:
        _sim = hostsim_util.sim_lib("onsetsim", pthread=True)
        c = ctypes
        _sim.onsetsim_exec.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_longlong, c.c_int, c.c_longlong, c.c_int, c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_void_p, c.c_int,
                                       c.c_int, c.c_longlong, c.c_longlong, c.c_int, c.c_double, c.c_double, c.c_void_p, c.c_int, c.c_void_p]
    return _sim


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def sim_exec(S, ref, job, code, pad, n_out, item_max=None, rows_only=False):
    """One lra_onset_exec through the simulator; S: (batch, n_bands, n_frames).  The output arrives full of NaN: every element must be stored."""
    S = np.ascontiguousarray(S)
    real = S.dtype
    batch, n_bands, n_frames = S.shape
    off = idx = None
    n_ch = widest = 0
    rows = n_bands
    if code not in (O._NONE, O._ROWS):
        job = dict(job)
        O._prepare_channels(job, n_bands)
        if job["tables"] is None:  # channels=None: no tables, one channel of every band
            n_ch, widest, rows = 1, n_bands, 1
        else:
            off, idx, widest = job["tables"]
            n_ch = rows = len(off) - 1
    detrend = job["detrend"] and code is not None
    out = np.full((batch, rows, n_out), np.nan, dtype=np.float64 if detrend else real)
    env = np.full((batch, rows, n_out), np.nan, dtype=real) if detrend else None
    ref = None if ref is None else np.ascontiguousarray(ref, dtype=real).reshape(S.shape)
    im = None if item_max is None else np.ascontiguousarray(item_max, dtype=real)
    rc = sim_lib().onsetsim_exec(_p(S), _p(ref), _p(out), batch, n_bands, n_frames, int(real == np.float64), job["lag"], job["max_size"], code, _p(off), _p(idx), n_ch, widest, pad,
                                 n_out, int(im is not None), 1e-10, 80.0, _p(im), int(detrend), _p(env))
    assert rc == 0
    return out


def sim_case(golden, name):
    """The case's envelope computed as onset.py drives the kernel, with the kernel bodies on host threads and the reference's own spectrogram as input."""
    case = json.loads(str(golden["cases"]))[name]
    kw = dict(case["kwargs"])
    agg = AGGREGATES[case["aggregate"]]
    lag, max_size, center = kw.get("lag", 1), kw.get("max_size", 1), kw.get("center", True)
    n_fft, hop = kw.get("n_fft", 2048), kw.get("hop_length", 512)
    channels = kw.get("channels")
    if isinstance(channels, dict):
        channels = [slice(a, b) for a, b in channels["slices"]]
    code = O._NONE
    if callable(agg):
        code = next((c for f, c in O._DEVICE_AGGREGATES if agg is f), None)
    job = dict(lag=lag, max_size=max_size, code=code, aggregate=agg, channels=channels, pad_width=lag + (n_fft // (2 * hop) if center else 0), center=center,
               detrend=bool(kw.get("detrend", False)))
    ref = None
    if case["mel"] is not None:  # power spectrogram in, decibels fused (the per-clip maximum of |mel| as lra_item_max_exec makes it)
        S = golden[f"mel_{case['mel']}"]
    elif "feature" in kw:
        S = np.abs(golden[f"feature_out_{name}"])
    else:
        S = np.atleast_2d(golden[case["input"]])
        if isinstance(kw.get("ref"), str):
            ref = golden[kw["ref"]]
    fuse = case["mel"] is not None or "feature" in kw
    lead = S.shape[:-2]
    S3 = S.reshape((-1,) + S.shape[-2:])
    item_max = np.abs(S3).reshape(S3.shape[0], -1).max(axis=1) if fuse else None
    n_frames = S3.shape[-1]
    n_env = max(n_frames - lag, 0)
    if code is None:  # the host callable: per-band flux, util.sync on the host, then the rows through the kernel's pad / trim / detrend
        flux = sim_exec(S3, ref, job, O._NONE, 0, n_env, item_max).reshape(lead + (S3.shape[1], n_env))
        agg_rows = O._sync_host(flux, job)
        A = agg_rows.reshape((-1,) + agg_rows.shape[-2:])
        n_out = O._out_frames(A.shape[-1], job, n_frames)
        out = sim_exec(A, None, dict(job, lag=1, max_size=1), O._ROWS, job["pad_width"], n_out)
        res = out.reshape(lead + out.shape[1:])
    else:
        n_out = O._out_frames(n_env, job, n_frames)
        out = sim_exec(S3, ref, job, code, job["pad_width"], n_out, item_max)
        res = out.reshape(lead + out.shape[1:])
    return res[..., 0, :] if case["fn"] == "strength" else res


@pytest.mark.parametrize("name", CASE_NAMES)
def test_kernel_bodies_reproduce_the_reference(golden, name):
    want = golden[name]
    got = sim_case(golden, name)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    if not ok.any():
        return
    scale = np.max(np.abs(want[ok]))
    err = np.max(np.abs(got[ok].astype(np.float64) - want[ok]))
    bound = (1e-12 if want.dtype == np.float64 and "f64" in name else 1e-5) * max(scale, 1e-30)
    assert err <= bound, f"{name}: max |err| {err:.3e} > {bound:.3e} (max |ref| {scale:.3e})"


def test_median_selects_exact_order_statistics():
    """The radix select against np.median on ties, zeros, odd and even counts (no decibel step: S is used as given)."""
    rng = np.random.default_rng(3)
    S = np.round(rng.standard_normal((2, 13, 300)) * 2.0).astype(np.float32)  # many ties and exact zeros after the rectification
    for channels in ([0, 1, 2, 5, 9, 13], [0, 13], [slice(0, 13, 3), slice(12, 0, -1)]):
        job = dict(lag=1, max_size=1, code=O._MEDIAN, aggregate=np.median, channels=channels, pad_width=1, center=False, detrend=False)
        got = sim_exec(S, None, job, O._MEDIAN, 1, 300)
        env = np.maximum(0.0, S[..., 1:] - S[..., :-1])
        slices = O._channel_slices(channels, 13)
        want = np.stack([np.median(env[:, s, :], axis=-2) for s in slices], axis=1)
        assert np.array_equal(got[..., 1:], want) and not got[..., 0].any()
