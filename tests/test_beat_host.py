"""beat_track without a GPU: argument checks before any device work, the converters against tests/golden/beat.npz, and the kernel bodies of
librosa_amd/csrc/lra_beat.h run on host threads (tests/hostsim/beatsim.cpp) on the reference's envelopes with the reference's BPM."""
import ctypes

import numpy as np
import pytest

import beat_signals as BS
import hostsim_util
import librosa_amd as L


@pytest.fixture(scope="module")
def golden():
    return BS.load()


# ---- argument checks: ParameterError before any device call (this host has no GPU: a device call would raise NativeError) ----------------
ENV = np.abs(np.random.default_rng(0).standard_normal(100)).astype(np.float32)


def test_an_input_is_required():
    with pytest.raises(L.ParameterError):
        L.beat.beat_track()


def test_sparse_needs_one_dimension():
    with pytest.raises(L.ParameterError):
        L.beat.beat_track(onset_envelope=np.stack([ENV, ENV]))
    with pytest.raises(L.ParameterError):  # from y the envelope's rank is y's rank
        L.beat.beat_track(y=np.zeros((2, 22050), np.float32))


@pytest.mark.parametrize("bpm", [0, -1, [120.0, 0.0], np.full(100, -3.0)])
def test_bpm_must_be_positive(bpm):
    with pytest.raises(L.ParameterError):
        L.beat.beat_track(onset_envelope=ENV, bpm=bpm)


@pytest.mark.parametrize("tightness", [0, -1])
def test_tightness_must_be_positive(tightness):
    with pytest.raises(L.ParameterError):
        L.beat.beat_track(onset_envelope=ENV, tightness=tightness)


def test_bpm_shape_must_match():
    with pytest.raises(L.ParameterError):
        L.beat.beat_track(onset_envelope=ENV, bpm=np.full(7, 120.0))
    with pytest.raises(L.ParameterError):
        L.beat.beat_track(onset_envelope=np.stack([ENV, ENV]), bpm=np.full((2, 7), 120.0), sparse=False)
    with pytest.raises(L.ParameterError):  # more dimensions than the envelope
        L.beat.beat_track(onset_envelope=ENV, bpm=np.full((2, 100), 120.0))


def test_units_are_checked_first():
    with pytest.raises(L.ParameterError):
        L.beat.beat_track(onset_envelope=ENV, units="bars")
    with pytest.raises(L.ParameterError):  # documented difference: the reference returns the empty result here
        L.beat.beat_track(onset_envelope=np.zeros(50, np.float32), units="bars")
    with pytest.raises(L.ParameterError):
        L.beat.beat_track(y=np.zeros(22050, np.float32), units="bars")


@pytest.mark.parametrize("hop", [0, None, -512, 512.5])
def test_hop_length_must_be_a_positive_integer(hop):
    with pytest.raises(L.ParameterError):  # also with a given envelope: the frame rate and the units need it
        L.beat.beat_track(onset_envelope=ENV, bpm=120.0, hop_length=hop)
    with pytest.raises(L.ParameterError):
        L.beat.beat_track(y=np.zeros(22050, np.float32), hop_length=hop)


def test_start_bpm_must_be_positive():
    with pytest.raises(L.ParameterError):
        L.beat.beat_track(onset_envelope=ENV, start_bpm=0)


def test_zero_envelope_needs_no_device(golden):
    z, _, inputs, _ = golden
    tempo, beats = L.beat.beat_track(onset_envelope=inputs["env_zero"])
    assert tempo == 0.0 and isinstance(tempo, float) and beats.shape == (0,) and beats.dtype == z["beats_zero_sparse"].dtype
    tempo, beats = L.beat.beat_track(onset_envelope=inputs["env_zero2"], sparse=False)
    assert np.array_equal(tempo, z["tempo_zero_dense"]) and tempo.dtype == np.float64
    assert np.array_equal(beats, z["beats_zero_dense"]) and beats.dtype == bool


def test_a_live_envelope_reaches_the_device():
    if L.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(L.NativeError):
        L.beat.beat_track(onset_envelope=ENV, bpm=120.0)


# ---- the converters -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,n_fft,sr", [(512, None, 22050), (160, 400, 16000), (441, 2048, 22050)])
def test_converters_match_the_reference(golden, hop, n_fft, sr):
    z, _, _, _ = golden
    fr, tm, sm = z["conv_frames"], z["conv_times"], z["conv_samples"]
    tag = f"{hop}_{n_fft}_{sr}"
    got = dict(frames_to_samples=L.frames_to_samples(fr, hop_length=hop, n_fft=n_fft), samples_to_frames=L.samples_to_frames(sm, hop_length=hop, n_fft=n_fft),
               frames_to_time=L.frames_to_time(fr, sr=sr, hop_length=hop, n_fft=n_fft), time_to_frames=L.time_to_frames(tm, sr=sr, hop_length=hop, n_fft=n_fft),
               samples_to_time=L.samples_to_time(sm, sr=sr), time_to_samples=L.time_to_samples(tm, sr=sr))
    for name, val in got.items():
        want = z[f"{name}_{tag}"]
        assert val.dtype == want.dtype and np.array_equal(val, want), name
    assert L.core.frames_to_time is L.frames_to_time and np.isscalar(L.frames_to_samples(3)) and L.time_to_frames(1.0) == 43


# ---- the kernel bodies on host threads ------------------------------------------------------------------------------------------------------
_sim = None


def sim_lib():
    global _sim
    if _sim is None:
        _sim = hostsim_util.sim_lib("beatsim", pthread=True)
        c = ctypes
        _sim.beatsim_exec.argtypes = [c.c_void_p, c.c_longlong, c.c_longlong, c.c_int, c.c_void_p, c.c_int, c.c_double, c.c_double, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p,
                                      c.c_void_p, c.POINTER(c.c_int)]
    return _sim


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def sim_exec(env, bpm, frame_rate, tightness=100, trim=True):
    """One lra_beat_exec through the simulator on (..., n) envelopes with ``bpm`` as beat_track takes it -> beats, local score, cum, backlink."""
    from librosa_amd import beat as B

    env = np.ascontiguousarray(env)
    lead, n = env.shape[:-1], env.shape[-1]
    batch = int(np.prod(lead)) if lead else 1
    rows, mode = B._expand_bpm(bpm, env.ndim, lead, n)
    out = np.full((batch, n), 0xFF, np.uint8)
    local = np.full((batch, n), np.nan, env.dtype)
    cum = np.full((batch, n), np.nan)
    bl = np.full((batch, n), -7, np.int32)
    flag = ctypes.c_int(0)
    rc = sim_lib().beatsim_exec(_p(env), batch, n, int(env.dtype == np.float64), _p(rows), mode, frame_rate, tightness, int(trim), _p(out), _p(local), _p(cum), _p(bl),
                                ctypes.byref(flag))
    assert rc == 0
    assert set(np.unique(out)) <= {0, 1}  # every element of the beat row is stored
    return out.reshape(lead + (n,)).astype(bool), local.reshape(lead + (n,)), cum.reshape(lead + (n,)), bl.reshape(lead + (n,)), bool(flag.value)


def _want_dense(z, name, shape):
    want = z[f"beats_{name}"]
    if want.dtype == bool:
        return want
    dense = np.zeros(shape, bool)
    dense[want] = True
    return dense


SIM_CASES = [n for n in BS.names() if not n.startswith(("zero_", "units_samples", "units_time"))]


@pytest.mark.parametrize("name", SIM_CASES)
def test_simulated_tracker_matches_the_reference(golden, name):
    z, cases, _, params = golden
    kw = BS.call_kwargs(cases[name]["kwargs"], z, name)
    env = z[f"env_{name}"]
    sr, hop = kw.get("sr", BS.SR), kw.get("hop_length", 512)
    bpm = kw["bpm"] if "bpm" in kw else z[f"tempo_{name}"]  # the stored BPM: the reference's own estimate where none was given
    beats, ls, cum, bl, alive = sim_exec(env, bpm, float(sr) / hop, kw.get("tightness", 100), kw.get("trim", True))
    assert alive
    radius = params["radius"]
    for got, key in ((ls, "ls"), (cum, "cum")):
        want = z[f"{key}_{name}"]
        assert got.dtype == want.dtype
        scale = np.max(np.abs(want))
        err = np.max(np.abs(got.astype(np.float64) - want)) / scale if scale > 0 else 0.0
        print(f"{name}: {key} error {err:.3g} of the maximum")
        assert err <= radius
    print(f"{name}: {int(np.sum(bl != z[f'bl_{name}']))} of {bl.size} back-links differ")
    if name in ("units_frames",):
        assert kw["units"] == "frames"
    np.testing.assert_array_equal(beats, _want_dense(z, name, env.shape))


def test_simulated_rows_the_reference_cannot_handle(golden):
    z, _, _, _ = golden
    env = z["env_env_f32"]
    want = _want_dense(z, "env_f32", env.shape)
    bpm = float(z["tempo_env_f32"][0])
    both = np.stack([env, np.zeros_like(env), env])
    beats, _, _, _, alive = sim_exec(both, bpm, BS.SR / 512)
    assert alive and np.array_equal(beats[0], want) and not beats[1].any() and np.array_equal(beats[2], want)
    beats, _, _, _, alive = sim_exec(np.array([[1.5]], np.float32), 120.0, BS.SR / 512)  # a single frame
    assert alive and beats.shape == (1, 1) and not beats.any()
    beats, _, _, _, _ = sim_exec(env, 60 * BS.SR / 512, BS.SR / 512)  # one frame per beat: below the tracker's range
    assert not beats.any()
    beats, _, _, _, alive = sim_exec(np.zeros(40, np.float32), 120.0, BS.SR / 512)
    assert not alive and not beats.any()
