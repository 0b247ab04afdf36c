"""beat_track on the MI355X against tests/golden/beat.npz (the unmodified reference's tempo and beats, every case demanded exactly), the
bit-equality properties, the rows the reference cannot handle, and 256 x 30 s click trains."""
import numpy as np
import pytest

import beat_signals as BS
import librosa_amd as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return BS.load()


def _torch():
    import torch

    return torch


def _same(got, want):
    assert np.asarray(got).dtype == np.asarray(want).dtype and np.asarray(got).shape == np.asarray(want).shape
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name", BS.names())
def test_every_case_matches_the_reference(golden, name):
    z, cases, inputs, params = golden
    kind, key = cases[name]["input"].split(":")
    kw = BS.call_kwargs(cases[name]["kwargs"], z, name)
    want_tempo, want_beats = z[f"tempo_{name}"], z[f"beats_{name}"]
    if kind == "y":
        # first the envelope: the certification radius must cover this hardware's envelope error three times over (else regenerate the
        # fixture with a larger radius; the equality below stays)
        env = L.onset.onset_strength(y=inputs[key], sr=kw.get("sr", BS.SR), hop_length=kw.get("hop_length", 512), aggregate=np.median)
        ref = z[f"env_{name}"]
        err, peak = float(np.max(np.abs(env.astype(np.float64) - ref))), float(np.max(np.abs(ref)))
        print(f"{name}: envelope error {err / peak:.3g} of the maximum (radius {params['radius']:g})")
        assert 3 * err <= params["radius"] * peak
        tempo, beats = L.beat.beat_track(y=inputs[key], **kw)
        _same(tempo, want_tempo)
        _same(beats, want_beats)
    tempo, beats = L.beat.beat_track(onset_envelope=z[f"env_{name}"] if kind != "raw" else inputs[key], **kw)
    if "bpm" in kw:
        assert tempo is kw["bpm"]
    elif name == "zero_sparse":
        assert tempo == 0.0 and isinstance(tempo, float)
    else:
        _same(tempo, want_tempo)
    _same(beats, want_beats)


def test_numpy_tensor_and_rows_one_at_a_time_agree(golden):
    z, _, inputs, _ = golden
    torch = _torch()
    y = inputs["pulses"]
    tempo, beats = L.beat.beat_track(y=y, sparse=False)
    t_tempo, t_beats = L.beat.beat_track(y=torch.from_numpy(y).cuda(), sparse=False)
    assert t_tempo.is_cuda and t_beats.is_cuda and t_beats.dtype == torch.bool and t_tempo.dtype == torch.float64
    assert np.array_equal(tempo, t_tempo.cpu().numpy()) and np.array_equal(beats, t_beats.cpu().numpy())
    for i in range(len(y)):
        tempo_i, beats_i = L.beat.beat_track(y=y[i], sparse=False)
        assert np.array_equal(tempo_i, tempo[i]) and np.array_equal(beats_i, beats[i])
    assert not np.array_equal(beats[0], beats[3])
    env = z["env_bpm_channel"]
    tempo, beats = L.beat.beat_track(onset_envelope=env, sparse=False)
    t_tempo, t_beats = L.beat.beat_track(onset_envelope=torch.from_numpy(env).cuda(), sparse=False)
    assert np.array_equal(tempo, t_tempo.cpu().numpy()) and np.array_equal(beats, t_beats.cpu().numpy())
    for i in range(len(env)):
        tempo_i, beats_i = L.beat.beat_track(onset_envelope=env[i], sparse=False)
        assert np.array_equal(tempo_i, tempo[i]) and np.array_equal(beats_i, beats[i])


def test_sparse_is_the_true_positions_and_units_relate(golden):
    _, _, inputs, _ = golden
    torch = _torch()
    y, sr, hop = inputs["y16"], 16000, 160
    tempo, b1 = L.beat.beat_track(y=y, sr=sr, hop_length=hop)
    _, dense = L.beat.beat_track(y=y, sr=sr, hop_length=hop, sparse=False)
    assert b1.dtype == np.int64 and np.array_equal(b1, np.flatnonzero(dense)) and len(b1) > 0
    t1 = L.frames_to_time(b1, sr=sr, hop_length=hop)
    for units in ("frames", "samples", "time"):
        _, b2 = L.beat.beat_track(y=y, sr=sr, hop_length=hop, units=units)
        t2 = {"time": b2, "samples": L.samples_to_time(b2, sr=sr), "frames": L.frames_to_time(b2, sr=sr, hop_length=hop)}[units]
        assert np.allclose(t1, t2)
        _, b3 = L.beat.beat_track(y=torch.from_numpy(y).cuda(), sr=sr, hop_length=hop, units=units)
        assert b3.is_cuda and np.allclose(b3.cpu().numpy(), b2)


def test_zero_envelope_on_the_device(golden):
    _, _, inputs, _ = golden
    torch = _torch()
    tempo, beats = L.beat.beat_track(onset_envelope=torch.from_numpy(inputs["env_zero2"]).cuda(), sparse=False)
    assert tempo.shape == (2,) and not tempo.any() and beats.shape == (2, 100) and beats.dtype == torch.bool and not beats.any()
    tempo, beats = L.beat.beat_track(y=np.zeros(22050, np.float32))
    assert tempo == 0.0 and beats.shape == (0,)


def test_rows_the_reference_cannot_handle(golden):
    z, _, _, _ = golden
    env, want = z["env_env_f32"], np.zeros(z["env_env_f32"].shape, bool)
    want[z["beats_env_f32"]] = True
    bpm = float(z["tempo_env_f32"][0])
    _, beats = L.beat.beat_track(onset_envelope=np.stack([env, np.zeros_like(env), env]), bpm=bpm, sparse=False)
    assert np.array_equal(beats[0], want) and not beats[1].any() and np.array_equal(beats[2], want)
    tempo, beats = L.beat.beat_track(onset_envelope=np.stack([env, np.zeros_like(env)]), sparse=False)  # and with the tempo estimated per row
    assert np.array_equal(beats[0], want) and not beats[1].any() and tempo[0, 0] == z["tempo_env_f32"][0]
    _, beats = L.beat.beat_track(onset_envelope=np.array([1.5], np.float32), bpm=120.0)  # a single frame
    assert beats.shape == (0,)
    _, beats = L.beat.beat_track(onset_envelope=env, bpm=60 * BS.SR / 512)  # one frame per beat: below the tracker's range
    assert beats.shape == (0,)


def test_full_size_256_clips_of_30_s(golden):
    z, _, _, params = golden
    torch = _torch()
    y = np.stack([BS.full_signal(i) for i in range(BS.FULL_ROWS)])
    yt = torch.from_numpy(y).cuda()
    tempo, beats = L.beat.beat_track(y=yt, sr=BS.SR, sparse=False)
    assert tempo.shape == (BS.FULL_ROWS, 1) and beats.shape == (BS.FULL_ROWS, 1 + y.shape[-1] // 512)
    tempo, beats = tempo.cpu().numpy(), beats.cpu().numpy()
    env = L.onset.onset_strength(y=yt, sr=BS.SR, aggregate=np.median).cpu().numpy()
    for i in BS.FULL_STORED:
        ref = z[f"full_env_{i}"]
        assert 3 * np.max(np.abs(env[i].astype(np.float64) - ref)) <= params["radius"] * np.max(np.abs(ref))
        np.testing.assert_array_equal(tempo[i], z[f"full_tempo_{i}"])
        np.testing.assert_array_equal(np.flatnonzero(beats[i]), z[f"full_beats_{i}"])
    n = beats.shape[-1]
    for i in range(BS.FULL_ROWS):
        b = np.flatnonzero(beats[i])
        fpb = np.round(BS.SR / 512 * 60.0 / tempo[i, 0])
        assert len(b) >= 2 and b[0] >= 0 and b[-1] < n and np.all(np.diff(b) > 0), i
        assert abs(np.median(np.diff(b)) - fpb) <= 1, (i, tempo[i, 0], b)
