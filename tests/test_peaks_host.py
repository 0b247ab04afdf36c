"""onset_detect, onset_backtrack and util.peak_pick without a GPU: argument checks before any device work, the empty results, the greedy
model against tests/golden/peaks.npz, and the kernel bodies of librosa_amd/csrc/lra_peaks.h run on host threads
(tests/hostsim/peaksim.cpp) against every fixture case."""
import ctypes

import numpy as np
import pytest

import hostsim_util
import librosa_amd as L
import peak_cases as PC
from librosa_amd.util import peaks as P

onset_detect, onset_backtrack, peak_pick = L.onset.onset_detect, L.onset.onset_backtrack, L.util.peak_pick


@pytest.fixture(scope="module")
def golden():
    return PC.load()


# ---- argument checks: ParameterError before any device call (this host has no GPU: a device call would raise NativeError) ----------------
ENV = np.abs(np.random.default_rng(0).standard_normal(100)).astype(np.float32)
GOOD = dict(pre_max=3, post_max=3, pre_avg=3, post_avg=5, delta=0.3, wait=4)


@pytest.mark.parametrize("bad", [dict(pre_max=-1), dict(pre_avg=-1), dict(delta=-0.1), dict(wait=-1), dict(post_max=0), dict(post_avg=0), dict(post_max=-2), dict(method="best")])
def test_peak_pick_ranges_and_method(bad):
    with pytest.raises(L.ParameterError):
        peak_pick(ENV, **dict(GOOD, **bad))
    with pytest.raises(L.ParameterError):
        onset_detect(onset_envelope=ENV, **bad)
    with pytest.raises(L.ParameterError):  # documented difference: the reference returns the empty result for an all-zero envelope
        onset_detect(onset_envelope=np.zeros(50, np.float32), **bad)
    with pytest.raises(L.ParameterError):
        onset_detect(y=np.zeros(22050, np.float32), **bad)


def test_peak_pick_sparse_needs_one_dimension():
    with pytest.raises(L.ParameterError):
        peak_pick(np.stack([ENV, ENV]), **GOOD)
    with pytest.raises(L.ParameterError):
        peak_pick(np.stack([ENV, ENV]), sparse=False, axis=2, **GOOD)
    with pytest.raises(TypeError):  # the window arguments are keyword-only and required, as in the reference
        peak_pick(ENV, pre_max=3)


def test_onset_detect_checks_come_first():
    with pytest.raises(L.ParameterError):
        onset_detect()
    with pytest.raises(L.ParameterError):
        onset_detect(onset_envelope=ENV, units="bars")
    with pytest.raises(L.ParameterError):
        onset_detect(y=np.zeros(22050, np.float32), units="bars")
    with pytest.raises(L.ParameterError):
        onset_detect(onset_envelope=ENV, backtrack=True, sparse=False)
    with pytest.raises(L.ParameterError):
        onset_detect(onset_envelope=np.stack([ENV, ENV]))
    with pytest.raises(L.ParameterError):  # from y the envelope's rank is y's rank
        onset_detect(y=np.zeros((2, 22050), np.float32))
    with pytest.raises(L.ParameterError):
        onset_detect(onset_envelope=ENV, backtrack=True, energy=np.stack([ENV, ENV]))
    with pytest.raises(TypeError):
        onset_detect(onset_envelope=ENV, tightness=3)
    onset_detect(onset_envelope=np.zeros(5, np.float32), units="bars", sparse=False)  # units are looked at with sparse=True only, as in the reference


@pytest.mark.parametrize("hop", [0, None, -512, 512.5])
def test_hop_length_must_be_a_positive_integer(hop):
    with pytest.raises(L.ParameterError):
        onset_detect(onset_envelope=ENV, hop_length=hop)


def test_integer_envelope_raises_as_the_in_place_division_does():
    env = np.arange(20)
    with pytest.raises(TypeError):
        onset_detect(onset_envelope=env)
    with pytest.raises(TypeError):
        onset_detect(onset_envelope=env.reshape(2, 10), sparse=False)


def test_onset_backtrack_checks(golden):
    z, _, inputs, _ = golden
    for name, (events, key) in PC.BACKTRACK.items():
        if z[f"back_{name}"].ndim == 0:  # the reference refuses the call
            assert str(z[f"back_{name}"]) == "ParameterError"
            with pytest.raises(L.ParameterError):
                onset_backtrack(np.asarray(events, dtype=np.int64), inputs[key])
    with pytest.raises(L.ParameterError):
        onset_backtrack(np.array([1, 2]), np.zeros((2, 30), np.float32))


def test_a_live_input_reaches_the_device():
    if L.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(L.NativeError):
        peak_pick(ENV, **GOOD)
    with pytest.raises(L.NativeError):
        onset_detect(onset_envelope=ENV)
    with pytest.raises(L.NativeError):
        onset_backtrack(np.array([3, 9]), ENV)


# ---- the results that need no device ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zero_sparse", "zero_time", "zero_dense", "const_dense", "inf_row", "inf_dense"])
def test_nothing_to_grab_needs_no_device(golden, name):
    z, cases, inputs, _ = golden
    env = inputs[cases[name]["input"].split(":")[1]]
    before = env.copy()
    got = onset_detect(onset_envelope=env, **PC.call_kwargs(cases[name]["kwargs"], inputs))
    want = z[f"onsets_{name}"]
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(env, before, equal_nan=True)


@pytest.mark.parametrize("name", ["len1", "len2"])
def test_short_energy_needs_no_device(golden, name):
    z, _, inputs, _ = golden
    events, key = PC.BACKTRACK[name]
    got = onset_backtrack(np.asarray(events), inputs[key])
    assert got.dtype == z[f"back_{name}"].dtype and np.array_equal(got, z[f"back_{name}"])


def test_empty_rows_need_no_device():
    assert peak_pick(np.zeros(0, np.float32), **GOOD).shape == (0,)
    assert peak_pick(np.zeros((3, 0), np.float32), sparse=False, **GOOD).shape == (3, 0)


def test_default_windows_follow_the_reference():
    # onset.py:184-189 at the two frame rates the fixture uses, after peak_pick's ceiling
    assert PC.detect_windows(22050, 512) == dict(pre_max=1, post_max=1, pre_avg=4, post_avg=5, wait=1, delta=0.07)
    assert PC.detect_windows(16000, 160) == dict(pre_max=3, post_max=1, pre_avg=10, post_avg=11, wait=3, delta=0.07)
    got = P.prepare(pre_max=2.5, post_max=2.2, pre_avg=3.7, post_avg=4.1, delta=0.25, wait=3.5)
    assert got == dict(pre_max=3, post_max=3, pre_avg=4, post_avg=5, delta=0.25, wait=4, method=0)


# ---- the greedy model against the reference -------------------------------------------------------------------------------------------------
def _dense(want, shape):
    if want.dtype == bool:
        return want
    out = np.zeros(shape, bool)
    out[want] = True
    return out


GREEDY_PICKS = [n for n, (_, kw) in PC.PICK.items() if kw.get("method", "greedy") == "greedy"]
GREEDY_DETECTS = [n for n, (src, kw) in PC.DETECT.items() if kw.get("method", "greedy") == "greedy" and not src.startswith("raw:") and not kw.get("backtrack") and "units" not in kw]


@pytest.mark.parametrize("name", GREEDY_PICKS)
def test_greedy_model_equals_the_fixture(golden, name):
    z, cases, inputs, _ = golden
    key, kw = PC.PICK[name]
    x = np.moveaxis(inputs[key], kw.get("axis", -1), -1)
    got = np.stack([PC.greedy_model(row, **PC.ceil_windows(kw)) for row in x.reshape(-1, x.shape[-1])]).reshape(x.shape)
    np.testing.assert_array_equal(np.moveaxis(got, -1, kw.get("axis", -1)), _dense(z[f"peaks_{name}"], inputs[key].shape))


@pytest.mark.parametrize("name", GREEDY_DETECTS)
def test_greedy_model_equals_the_detect_fixture(golden, name):
    z, _, _, _ = golden
    src, kw = PC.DETECT[name]
    env = z[f"env_{name}"]
    rows = PC.normalized(env) if kw.get("normalize", True) else env
    pick = dict(PC.detect_windows(kw.get("sr", PC.SR), kw.get("hop_length", 512)), **{k: v for k, v in kw.items() if k in ("pre_max", "post_max", "pre_avg", "post_avg", "wait", "delta")})
    got = np.stack([PC.greedy_model(row, **PC.ceil_windows(pick)) for row in rows.reshape(-1, rows.shape[-1])]).reshape(rows.shape)
    np.testing.assert_array_equal(got, _dense(z[f"onsets_{name}"], env.shape))


# ---- the kernel bodies on host threads ------------------------------------------------------------------------------------------------------
_sim = None


def sim_lib():
    global _sim
    if _sim is None:
        _sim = hostsim_util.sim_lib("peaksim", pthread=True)
        c = ctypes
        _sim.peaksim_pick.argtypes = [c.c_void_p, c.c_longlong, c.c_longlong, c.c_int, c.c_int, c.c_longlong, c.c_longlong, c.c_longlong, c.c_longlong, c.c_double, c.c_longlong, c.c_int,
                                      c.c_void_p, c.c_void_p, c.c_void_p, c.POINTER(c.c_int)]
        _sim.peaksim_prev_minimum.argtypes = [c.c_void_p, c.c_longlong, c.c_longlong, c.c_int, c.c_void_p]
    return _sim


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def sim_pick(x, kw, normalize=False):
    """One lra_peak_pick_exec through the simulator on (..., n) rows -> peaks, normalised rows, (some entry non-zero, every entry finite)."""
    x = np.ascontiguousarray(x)
    lead, n = x.shape[:-1], x.shape[-1]
    batch = int(np.prod(lead)) if lead else 1
    p = P.prepare(**{k: v for k, v in kw.items() if k in ("pre_max", "post_max", "pre_avg", "post_avg", "delta", "wait", "method")})
    out = np.full((batch, n), 0xFF, np.uint8)
    cand = np.full((batch, n), 0xFF, np.uint8)
    norm = np.full((batch, n), np.nan, x.dtype)
    flag = ctypes.c_int(0)
    rc = sim_lib().peaksim_pick(_p(x), batch, n, int(x.dtype == np.float64), int(normalize), p["pre_max"], p["post_max"], p["pre_avg"], p["post_avg"], p["delta"], p["wait"],
                                p["method"], _p(out), _p(norm), _p(cand), ctypes.byref(flag))
    assert rc == 0
    assert set(np.unique(out)) <= {0, 1} and set(np.unique(cand)) <= {0, 1}  # every element is stored
    return out.reshape(lead + (n,)).astype(bool), norm.reshape(lead + (n,)), (bool(flag.value & 1), bool(flag.value & 2))


def sim_prev_minimum(energy):
    energy = np.ascontiguousarray(energy)
    lead, m = energy.shape[:-1], energy.shape[-1]
    batch = int(np.prod(lead)) if lead else 1
    out = np.full((batch, m), -7, np.int32)
    assert sim_lib().peaksim_prev_minimum(_p(energy), batch, m, int(energy.dtype == np.float64), _p(out)) == 0
    return out.reshape(lead + (m,))


def test_the_case_table_knows_the_kernel_sizes():
    lib = sim_lib()
    assert (lib.peaksim_tile(), lib.peaksim_halo(), lib.peaksim_ring()) == (PC.TILE, PC.HALO, PC.RING)


@pytest.mark.parametrize("name", list(PC.PICK))
def test_simulated_picker_matches_the_reference(golden, name):
    z, _, inputs, _ = golden
    key, kw = PC.PICK[name]
    x = np.moveaxis(inputs[key], kw.get("axis", -1), -1)
    peaks, norm, _ = sim_pick(x, kw)
    assert np.array_equal(norm, x, equal_nan=True)  # normalize = 0: a copy
    np.testing.assert_array_equal(np.moveaxis(peaks, -1, kw.get("axis", -1)), _dense(z[f"peaks_{name}"], inputs[key].shape))


@pytest.mark.parametrize("name", list(PC.DETECT))
def test_simulated_detection_matches_the_reference(golden, name):
    z, _, inputs, _ = golden
    src, kw = PC.DETECT[name]
    kind, key = src.split(":")
    env = inputs[key] if kind == "raw" else z[f"env_{name}"]
    sr, hop = kw.get("sr", PC.SR), kw.get("hop_length", 512)
    pick = dict(PC.detect_windows(sr, hop), **{k: v for k, v in kw.items() if k in ("pre_max", "post_max", "pre_avg", "post_avg", "wait", "delta", "method")})
    normalize = kw.get("normalize", True)
    peaks, norm, (nonzero, finite) = sim_pick(env, pick, normalize=normalize)
    with np.errstate(invalid="ignore"):
        want_norm = PC.normalized(env) if normalize else env
    assert norm.dtype == want_norm.dtype and np.array_equal(norm.view(np.uint8), np.ascontiguousarray(want_norm).view(np.uint8))  # bit for bit
    assert nonzero == bool(want_norm.any()) and finite == bool(np.all(np.isfinite(want_norm)))
    want = z[f"onsets_{name}"]
    if not (nonzero and finite):
        assert want.size == 0 or not want.any()
        return
    if not kw.get("sparse", True):
        np.testing.assert_array_equal(peaks, want)
        return
    events = np.flatnonzero(peaks)
    if kw.get("backtrack"):
        energy = inputs[kw["energy"]] if "energy" in kw else norm
        prev = sim_prev_minimum(energy)
        if "energy" not in kw:
            np.testing.assert_array_equal(prev, z[f"prev_{name}"])
        events = prev[np.minimum(events, len(prev) - 1)]
    if kw.get("units") == "samples":
        events = L.frames_to_samples(events, hop_length=hop)
    elif kw.get("units") == "time":
        events = L.frames_to_time(events, hop_length=hop, sr=sr)
    np.testing.assert_array_equal(events, want)


@pytest.mark.parametrize("key", sorted({k for _, k in PC.BACKTRACK.values()} | {"energy300"}))
def test_simulated_preceding_minima_match_the_reference(golden, key):
    z, _, inputs, _ = golden
    prev = sim_prev_minimum(inputs[key])
    np.testing.assert_array_equal(prev, z[f"prev_{key}"])
    for name, (events, k) in PC.BACKTRACK.items():
        if k == key and z[f"back_{name}"].ndim:
            ev = np.asarray(events, dtype=np.int64)
            np.testing.assert_array_equal(prev[np.minimum(ev, len(prev) - 1)], z[f"back_{name}"])


def test_simulated_row_alone_equals_the_row_in_a_batch(golden):
    _, _, inputs, _ = golden
    for key, kw in (("b32_3x257", PC.PICK["batch_3x257"][1]), ("b64_2x2x90", PC.PICK["batch_2x2x90_dp_value"][1])):
        x = inputs[key].reshape(-1, inputs[key].shape[-1])
        peaks, norm, _ = sim_pick(x, kw, normalize=True)
        prev = sim_prev_minimum(norm)
        for i, row in enumerate(x):
            p1, n1, _ = sim_pick(row, kw, normalize=True)
            assert np.array_equal(p1, peaks[i]) and np.array_equal(n1, norm[i]) and np.array_equal(sim_prev_minimum(n1), prev[i])
        assert peaks.any() and not np.array_equal(peaks[0], peaks[1])


def test_simulated_status_is_over_the_whole_array(golden):
    _, _, inputs, _ = golden
    kw = dict(PC.detect_windows(PC.SR, 512))
    _, _, status = sim_pick(inputs["env_inf2"], kw, normalize=True)
    assert status == (True, False)
    _, _, status = sim_pick(np.stack([inputs["env_zero"], inputs["energy300"][:100]]), kw, normalize=True)
    assert status == (True, True)
    _, norm, status = sim_pick(inputs["env_const2"], kw, normalize=True)
    assert status == (False, True) and not norm.any()
