"""The edge-case table of tests/rhythm_edges.py on the MI355X through the public functions, NumPy in and device tensors in (the same bits),
against oracle/rhythm_oracle.py: all 25 transform sizes of the tempogram kernel and the direct kernel in WRITE, SUM and ARGMAX, the tiled and
untiled WRITE epilogue, the two refusals before launch, the beat tracker's ring wrap, its 2048 boundary and its half-even roundings, the
median kernel at 64 down to 1 frames per workgroup and at exactly 160 KiB of LDS, and the flux and detrend tile remainders."""
import numpy as np
import pytest

import librosa_amd as L
import rhythm_cases as RC
import rhythm_edges as E
import rhythm_oracle as O

pytestmark = pytest.mark.gpu

# The project's bound for a tempogram from a given envelope (tests/test_rhythm_gpu.py); the reference's own difference is 8.7e-16, the host
# simulator's worst 8.4e-15 (the direct kernel).  A device value above 1e-13 would be a finding, not a reason to widen this.
TG_ENV_BOUND = 1e-12
# Measured on the MI355X, the worst WRITE case per transform size as a fraction of the column maximum (profiles/rhythm_edges.md; the oracle's
# own numpy.fft rounding is of the same order, so these are upper bounds of the device's error):
#   direct 8.44e-15
#   N  160 9.72e-16    200 5.55e-16    240 5.55e-16    320 5.60e-16    400 5.78e-16    480 6.23e-16    600 6.66e-16    640 5.55e-16
#      720 5.55e-16    800 7.77e-16    882 1.08e-15    960 6.66e-16   1000 5.55e-16   1200 7.77e-16   1280 6.66e-16   1440 6.66e-16
#     1600 7.77e-16   1764 8.05e-16   1920 8.88e-16   2000 9.99e-16   2400 1.11e-15   2646 1.22e-15   3200 3.55e-15   3528 1.11e-15
#     4800 8.88e-16


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _both(fn, x, **kw):
    """fn on the NumPy array and on the device tensor: a NumPy result, and the same bits from the device path."""
    host = fn(x, **kw)
    dev = fn(_dev(x), **kw)
    assert isinstance(host, np.ndarray) and dev.is_cuda
    out = dev.cpu().numpy()
    assert out.dtype == host.dtype and np.array_equal(out, host, equal_nan=True)
    return host


# ---- tempogram / tempo ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.TG_CASES))
def test_tempogram_sizes_match_the_oracle(name):
    case = E.TG_CASES[name]
    env, W = E.tg_envelope(case), case["W"]
    norm = E.NORMS[case["norm"]]
    want = O.tempogram(env, win_length=W, center=case["center"], norm=norm)
    got = _both(lambda e: L.feature.tempogram(onset_envelope=e, win_length=W, center=case["center"], norm=norm), env)
    assert got.shape == want.shape and got.dtype == np.float64 and not np.isnan(got).any()
    err = RC.col_err(got, want)
    print(f"tempogram {name}: N = {E.transform_length(W)}, error {err:.3g} of the column maximum")
    assert err <= TG_ENV_BOUND
    if E.SUM not in case["modes"]:
        return
    for agg in (np.mean, None):  # the SUM and the ARGMAX epilogue
        want, margin = O.tempo(env, aggregate=agg, **E.tempo_kwargs(case))
        got = _both(lambda e: L.feature.tempo(onset_envelope=e, aggregate=agg, **E.tempo_kwargs(case)), env)
        assert got.shape == want.shape and got.dtype == np.float64
        ok = margin >= 1e-9
        assert ok.mean() >= 0.9
        np.testing.assert_array_equal(got[ok], want[ok])


def _ordinary_call_is_right():
    case = E.TG_CASES["n800_w400"]
    env = E.tg_envelope(case)
    got = L.feature.tempogram(onset_envelope=env, win_length=case["W"])
    assert RC.col_err(got, O.tempogram(env, win_length=case["W"])) <= TG_ENV_BOUND


def test_a_window_that_does_not_fit_is_refused_before_launch():
    env = np.abs(np.random.default_rng(1).standard_normal(20)).astype(np.float32)
    W = E.first_refused(E.WRITE)
    with pytest.raises(L.ParameterError, match="does not fit"):
        L.feature.tempogram(onset_envelope=env, win_length=W)
    _ordinary_call_is_right()
    W = E.first_refused(E.SUM)  # the running sums make the SUM layout larger: refused from a smaller window on
    with pytest.raises(L.ParameterError, match="does not fit"):
        L.feature.tempo(onset_envelope=env, sr=W, hop_length=1, ac_size=1.0)
    _ordinary_call_is_right()
    assert L.feature.tempogram(onset_envelope=env, win_length=W).shape == (W, 20)  # WRITE still fits at that window


# ---- beat tracker -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.BEAT_CASES))
def test_beat_edges_match_the_oracle(name):
    case = E.BEAT_CASES[name]
    env, bpm = E.beat_inputs(case)
    want = O.beat_track(env, bpm=bpm, frame_rate=E.FRAME_RATE, tightness=case["tightness"], trim=case["trim"])[0]
    got = _both(lambda e: L.beat.beat_track(onset_envelope=e, bpm=bpm, tightness=case["tightness"], trim=case["trim"], sparse=False, **E.BEAT_KW)[1], env)
    assert got.dtype == bool
    np.testing.assert_array_equal(got, want)
    live = env.reshape(-1, env.shape[-1]).any(axis=-1).reshape(env.shape[:-1])
    assert got[live].any(axis=-1).all() and not got[~live].any()


# ---- onset strength ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.ONSET_CASES))
def test_onset_edges_match_the_oracle(name):
    case = E.ONSET_CASES[name]
    S = E.onset_input(case)
    kw = E.onset_kwargs(case)
    got = _both(lambda s: L.onset.onset_strength_multi(S=s, **kw), S)
    E.check_onset(case, got, S, lambda: L.onset.onset_strength_multi(S=S, **dict(kw, detrend=False)))


def test_a_median_channel_that_does_not_fit_is_refused_before_launch():
    S = np.abs(np.random.default_rng(2).standard_normal((E.ONSET_REFUSED_BANDS, 3))).astype(np.float32)
    with pytest.raises(L.ParameterError, match="does not fit"):
        L.onset.onset_strength_multi(S=S, aggregate=np.median)
    case = E.ONSET_CASES["median_f32_257"]
    S = E.onset_input(case)
    E.check_onset(case, L.onset.onset_strength_multi(S=S, **E.onset_kwargs(case)), S, None)
