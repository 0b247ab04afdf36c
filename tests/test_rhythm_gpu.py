"""tempogram / tempo on the MI355X against tests/golden/rhythm.npz, bit-equality properties, and 256 x 30 s against a float64 numpy.fft
restatement of the autocorrelation built from this package's own envelope."""
import numpy as np
import pytest

import librosa_amd as L
import rhythm_cases as RC

pytestmark = pytest.mark.gpu

# measured on the MI355X (see the pull request): from the reference's envelope float64 rounding only; from y the float32 envelope's own error
TG_ENV_BOUND = 1e-12
TG_Y_BOUND = 5e-5  # measured 6.3e-8 (tg_16k); from the reference envelope 8.7e-16 (tg_norm_1)


@pytest.fixture(scope="module")
def golden():
    return RC.load()


def _torch():
    import torch

    return torch


def _call(z, cases, inputs, name, use_ref_env):
    case = cases[name]
    call = RC.call_kwargs(case["kwargs"], inputs)
    fn = getattr(L.feature, case["fn"])
    src = case["input"]
    if case["fn"] == "tempo" and src.startswith("tg:"):
        tg = L.feature.tempogram(onset_envelope=z[f"env_{name}"], sr=call.get("sr", RC.SR), hop_length=call.get("hop_length", 512))
        return fn(tg=tg, **call)
    if use_ref_env or not RC.from_signal(case):
        return fn(onset_envelope=z[f"env_{name}"], **call)
    return fn(y=inputs[src], **call)


@pytest.mark.parametrize("name", RC.names("tempogram"))
def test_tempogram_from_the_reference_envelope(golden, name):
    z, cases, inputs = golden
    got = _call(z, cases, inputs, name, True)
    assert got.dtype == np.float64
    err = RC.col_err(RC.sampled(z, name, got), z[name])
    print(f"{name}: {err:.3g}")
    assert err <= TG_ENV_BOUND


@pytest.mark.parametrize("name", [n for n in RC.names("tempogram") if n in ("tg_y_stereo", "tg_y_f64", "tg_hop441", "tg_16k")])
def test_tempogram_from_y(golden, name):
    z, cases, inputs = golden
    got = _call(z, cases, inputs, name, False)
    assert got.shape[:-1] == z[name].shape[:-1] and got.dtype == np.float64
    err = RC.col_err(RC.sampled(z, name, got), z[name])
    print(f"{name}: {err:.3g}")
    assert err <= TG_Y_BOUND


@pytest.mark.parametrize("name", RC.names("tempo"))
def test_tempo_matches_the_reference(golden, name):
    z, cases, inputs = golden
    want, margin = z[name], z[f"margin_{name}"].reshape(z[name].shape)
    for use_ref_env in (True, False):
        got = _call(z, cases, inputs, name, use_ref_env)
        assert got.shape == want.shape and got.dtype == np.float64
        exact_env = use_ref_env or not RC.from_signal(cases[name]) or name == "tempo_silent"  # (silence: the envelope is exactly zero either way)
        ok = margin >= (1e-9 if exact_env else 1e-3)
        assert ok.mean() >= 0.9
        np.testing.assert_array_equal(got[ok], want[ok])


def test_nonfinite_envelope_raises_for_every_norm():
    env = np.ones(200, np.float32)
    env[50] = np.inf
    for norm in (np.inf, None, 1, 2, 3):
        with pytest.raises(L.ParameterError, match="finite"):
            L.feature.tempogram(onset_envelope=env, norm=norm)
    t = _torch().from_numpy(env).cuda()
    with pytest.raises(L.ParameterError, match="finite"):
        L.feature.tempo(onset_envelope=t)


def test_device_tensors_in_give_the_same_bits(golden):
    z, _, inputs = golden
    torch = _torch()
    env = z["env_tempo_env"]
    for kw in (dict(), dict(win_length=127, norm=2), dict(win_length=64, center=False)):
        a = L.feature.tempogram(onset_envelope=env, **kw)
        b = L.feature.tempogram(onset_envelope=torch.from_numpy(env).cuda(), **kw)
        assert b.is_cuda and np.array_equal(a, b.cpu().numpy())
    for agg in (np.mean, None):
        a = L.feature.tempo(onset_envelope=env, aggregate=agg)
        b = L.feature.tempo(onset_envelope=torch.from_numpy(env).cuda(), aggregate=agg)
        assert b.is_cuda and np.array_equal(a, b.cpu().numpy())
    y = inputs["y"]
    assert np.array_equal(L.feature.tempo(y=y), L.feature.tempo(y=torch.from_numpy(y).cuda()).cpu().numpy())


def test_a_batch_equals_each_item_alone(golden):
    z, _, inputs = golden
    env = np.concatenate([z["env_tempo_env"], z["env_tempo_pulses"][:, : z["env_tempo_env"].shape[-1]]])
    for agg in (np.mean, None):
        batch = L.feature.tempo(onset_envelope=env, aggregate=agg)
        for i in range(len(env)):
            assert np.array_equal(batch[i], L.feature.tempo(onset_envelope=env[i], aggregate=agg))
    tg = L.feature.tempogram(onset_envelope=env)
    for i in range(len(env)):
        assert np.array_equal(tg[i], L.feature.tempogram(onset_envelope=env[i]))


def test_from_y_equals_from_this_package_envelope(golden):
    _, _, inputs = golden
    y = inputs["pulses"]
    env = L.onset.onset_strength(y=y)
    assert np.array_equal(L.feature.tempo(y=y), L.feature.tempo(onset_envelope=env))
    assert np.array_equal(L.feature.tempo(y=y, aggregate=None), L.feature.tempo(onset_envelope=env, aggregate=None))
    assert np.array_equal(L.feature.tempogram(y=y), L.feature.tempogram(onset_envelope=env))


def test_fourier_tempogram_is_the_envelope_stft(golden):
    z, _, _ = golden
    env = z["env_tempo_env"]
    F = L.feature.fourier_tempogram(onset_envelope=env, win_length=128)
    D = L.stft(env, n_fft=128, hop_length=1)
    assert F.shape == D.shape and np.array_equal(F, D)


def _restated(env, W):
    """float64 numpy.fft restatement of tempogram(onset_envelope=env, win_length=W) for (n,) env."""
    n = env.shape[-1]
    p = np.pad(env, (W // 2, W // 2), mode="linear_ramp", end_values=0).astype(np.float64)
    fr = np.lib.stride_tricks.sliding_window_view(p, W)[:n].T * L.filters.get_window("hann", W, fftbins=True)[:, None]
    N = 2 * W
    ac = np.fft.irfft(np.abs(np.fft.rfft(fr, n=N, axis=0)) ** 2, n=N, axis=0)[:W]
    m = np.max(np.abs(ac), axis=0, keepdims=True)
    return ac / np.where(m < np.finfo(np.float64).tiny, 1.0, m)


def test_full_size_256_clips_of_30_s():
    torch = _torch()
    g = torch.Generator(device="cuda").manual_seed(5)
    y = torch.randn((256, 30 * 22050), generator=g, device="cuda", dtype=torch.float32) * 0.1
    t = torch.arange(30 * 22050, device="cuda")
    y = y * (1.0 + 3.0 * ((t % 11025) < 600))
    env = L.onset.onset_strength(y=y)
    tg = L.feature.tempogram(y=y)
    assert tg.shape == (256, 384, env.shape[-1]) and tg.dtype == torch.float64
    bpm = L.feature.tempo(y=y)
    per_frame = L.feature.tempo(y=y, aggregate=None)
    assert bpm.shape == (256, 1) and per_frame.shape == (256, env.shape[-1])
    e = env.cpu().numpy()
    for i in (0, 77, 190, 255):
        want = _restated(e[i], 384)
        err = RC.col_err(tg[i].cpu().numpy(), want)
        print(f"clip {i}: {err:.3g}")
        assert err <= 1e-12
    assert np.array_equal(bpm.cpu().numpy(), L.feature.tempo(onset_envelope=env).cpu().numpy())
