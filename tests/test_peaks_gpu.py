"""onset_detect, onset_backtrack and util.peak_pick on the MI355X against tests/golden/peaks.npz (the unmodified reference's results, every
case demanded exactly: each is certified by scripts/make_peak_golden.py or exact by arithmetic), the agreement of NumPy input, device tensors
and rows one at a time, and 256 x 30 s click trains against the greedy model.

Measured on the MI355X: the device's envelope lies within 3.65e-7 of the maximum of the reference's on every case that starts from a signal
(y_16k; the stored full-size rows 2.43e-7 at most, float64 2.4e-16), against the certification radius of 1e-5."""
import numpy as np
import pytest

import librosa_amd as L
import peak_cases as PC

pytestmark = pytest.mark.gpu

onset_detect, onset_backtrack, peak_pick = L.onset.onset_detect, L.onset.onset_backtrack, L.util.peak_pick


@pytest.fixture(scope="module")
def golden():
    return PC.load()


def _torch():
    import torch

    return torch


def _same(got, want):
    assert np.asarray(got).dtype == np.asarray(want).dtype and np.asarray(got).shape == np.asarray(want).shape
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name", list(PC.PICK))
def test_every_peak_pick_case_matches_the_reference(golden, name):
    z, _, inputs, _ = golden
    key, kw = PC.PICK[name]
    x = inputs[key]
    before = x.copy()
    _same(peak_pick(x, **kw), z[f"peaks_{name}"])
    got = peak_pick(_torch().from_numpy(x).cuda(), **kw)
    assert got.is_cuda
    _same(got.cpu().numpy(), z[f"peaks_{name}"])
    assert np.array_equal(x, before, equal_nan=True)


def _envelope_is_within_the_radius(name, env, ref, radius):
    """The certification radius must cover this hardware's envelope error three times over (else regenerate the fixture with a larger radius;
    the equality that follows stays)."""
    err, peak = float(np.max(np.abs(np.asarray(env, dtype=np.float64) - ref))), float(np.max(np.abs(ref)))
    print(f"{name}: envelope error {err / peak:.3g} of the maximum (radius {radius:g})")
    assert 3 * err <= radius * peak


@pytest.mark.parametrize("name", list(PC.DETECT))
def test_every_onset_detect_case_matches_the_reference(golden, name):
    z, cases, inputs, params = golden
    src, kw = PC.DETECT[name]
    kind, key = src.split(":")
    call = PC.call_kwargs(kw, inputs)
    want = z[f"onsets_{name}"]
    if kind == "y":
        assert cases[name]["certified"]
        env = L.onset.onset_strength(y=inputs[key], sr=kw.get("sr", PC.SR), hop_length=kw.get("hop_length", 512))
        _envelope_is_within_the_radius(name, env, z[f"env_{name}"], params["radius"])
        _same(onset_detect(y=inputs[key], **call), want)
        got = onset_detect(y=_torch().from_numpy(inputs[key]).cuda(), **call)
        assert got.is_cuda
        _same(got.cpu().numpy(), want)
    env = inputs[key] if kind == "raw" else z[f"env_{name}"]
    before = env.copy()
    _same(onset_detect(onset_envelope=env, **call), want)
    assert np.array_equal(env, before, equal_nan=True)
    got = onset_detect(onset_envelope=_torch().from_numpy(env).cuda(), **call)  # also the zero and the non-finite envelopes
    assert got.is_cuda
    _same(got.cpu().numpy(), want)


@pytest.mark.parametrize("name", list(PC.BACKTRACK))
def test_onset_backtrack_matches_the_reference(golden, name):
    z, _, inputs, _ = golden
    torch = _torch()
    events, key = PC.BACKTRACK[name]
    ev, energy, want = np.asarray(events, dtype=np.int64), inputs[key], z[f"back_{name}"]
    if want.ndim == 0:
        with pytest.raises(L.ParameterError):
            onset_backtrack(torch.from_numpy(ev).cuda(), torch.from_numpy(energy).cuda())
        return
    _same(onset_backtrack(ev, energy), want)
    got = onset_backtrack(torch.from_numpy(ev).cuda(), torch.from_numpy(energy).cuda())
    assert got.is_cuda
    _same(got.cpu().numpy(), want)
    _same(onset_backtrack(ev, torch.from_numpy(energy).cuda()).cpu().numpy(), want)
    _same(onset_backtrack(ev.reshape(1, -1), energy), want.reshape(1, -1))  # the result has events.shape


def test_numpy_tensor_and_rows_one_at_a_time_agree(golden):
    z, _, inputs, _ = golden
    torch = _torch()
    y = inputs["pulses"]
    dense = onset_detect(y=y, sparse=False)
    t_dense = onset_detect(y=torch.from_numpy(y).cuda(), sparse=False)
    assert dense.dtype == bool and t_dense.is_cuda and t_dense.dtype == torch.bool and np.array_equal(dense, t_dense.cpu().numpy())
    for i in range(len(y)):
        assert np.array_equal(onset_detect(y=y[i], sparse=False), dense[i])
        assert np.array_equal(onset_detect(y=y[i]), np.flatnonzero(dense[i]))
    assert not np.array_equal(dense[0], dense[3])
    for key, kw in (("b32_3x257", PC.PICK["batch_3x257"][1]), ("b64_2x2x90", PC.PICK["batch_2x2x90_dp_value"][1])):
        x = inputs[key]
        rows = peak_pick(x, **kw)
        for idx in np.ndindex(*x.shape[:-1]):
            assert np.array_equal(peak_pick(x[idx], **kw), rows[idx])
            assert np.array_equal(onset_detect(onset_envelope=x[idx], sparse=False, method=kw.get("method", "greedy")),
                                  onset_detect(onset_envelope=x, sparse=False, method=kw.get("method", "greedy"))[idx])


def test_sparse_is_the_true_positions_and_units_relate(golden):
    _, _, inputs, _ = golden
    torch = _torch()
    y, sr, hop = inputs["y16"], 16000, 160
    b1 = onset_detect(y=y, sr=sr, hop_length=hop)
    dense = onset_detect(y=y, sr=sr, hop_length=hop, sparse=False)
    assert b1.dtype == np.int64 and np.array_equal(b1, np.flatnonzero(dense)) and len(b1) > 0
    t1 = L.frames_to_time(b1, sr=sr, hop_length=hop)
    for units in ("frames", "samples", "time"):
        b2 = onset_detect(y=y, sr=sr, hop_length=hop, units=units)
        t2 = {"time": b2, "samples": L.samples_to_time(b2, sr=sr), "frames": L.frames_to_time(b2, sr=sr, hop_length=hop)}[units]
        assert np.allclose(t1, t2)
        b3 = onset_detect(y=torch.from_numpy(y).cuda(), sr=sr, hop_length=hop, units=units)
        assert b3.is_cuda and np.allclose(b3.cpu().numpy(), b2)
    x = inputs["r32_1292_10"]
    kw = PC.PICK["greedy_f32_1292"][1]
    assert np.array_equal(peak_pick(x, **kw), np.flatnonzero(peak_pick(x, sparse=False, **kw)))


def test_nothing_to_grab_on_the_device(golden):
    _, _, inputs, _ = golden
    torch = _torch()
    got = onset_detect(onset_envelope=torch.from_numpy(inputs["env_zero2"]).cuda(), sparse=False)
    assert got.is_cuda and got.shape == (2, 100) and got.dtype == torch.bool and not got.any()
    got = onset_detect(onset_envelope=torch.from_numpy(inputs["env_inf"]).cuda(), units="time")
    assert got.is_cuda and got.shape == (0,) and got.dtype == torch.float64
    got = onset_detect(y=np.zeros(22050, np.float32))
    assert got.shape == (0,) and got.dtype == np.int64
    got = onset_detect(y=torch.zeros(2, 22050).cuda(), sparse=False)
    assert got.shape == (2, 44) and not got.any()
    with pytest.raises(L.ParameterError):  # a live envelope without a peak: the reference's match_events refuses the empty event list
        onset_detect(onset_envelope=np.arange(20, dtype=np.float32)[::-1].copy(), backtrack=True, delta=5.0)


def test_full_size_256_clips_of_30_s(golden):
    z, _, _, params = golden
    torch = _torch()
    y = np.stack([PC.full_signal(i) for i in range(PC.FULL_ROWS)])
    yt = torch.from_numpy(y).cuda()
    dense = onset_detect(y=yt, sr=PC.SR, sparse=False)
    assert dense.is_cuda and dense.shape == (PC.FULL_ROWS, 1 + y.shape[-1] // 512)
    dense = dense.cpu().numpy()
    env = L.onset.onset_strength(y=yt, sr=PC.SR).cpu().numpy()
    for i in PC.FULL_STORED:
        _envelope_is_within_the_radius(f"full {i}", env[i], z[f"full_env_{i}"], params["radius"])
        np.testing.assert_array_equal(np.flatnonzero(dense[i]), z[f"full_onsets_{i}"])
    # every row against the greedy model on the device's own envelope: the normalisation is bit-identical and both means are float64
    pick = PC.detect_windows(PC.SR, 512)
    norm = PC.normalized(env)
    for i in range(PC.FULL_ROWS):
        np.testing.assert_array_equal(dense[i], PC.greedy_model(norm[i], **pick), err_msg=f"row {i}")
        assert dense[i].sum() >= 10
