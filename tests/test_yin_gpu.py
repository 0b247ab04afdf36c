"""yin and _yin_frames on the MI355X against tests/golden/yin.npz (the unmodified reference) and the float64 model of tests/yin_cases.py,
under that module's rules: silent frames exact; on settled frames the reference's lag, f0 within 16 x the reference's own distance from the
exact evaluation (at least 4 float64 ulp) of the float64 model and, for float32 samples, within twice the reference's float32 distance; the
dense CMND under the same two rules and the shifts within what the CMND's bound allows.

Shapes are the smallest at which the kernels can go wrong (tests/yin_cases.py): frame lengths 64, 512, 1001, 2048, 4500 and 8192 (the last two: the
direct kernel), transform lengths 160, 800, 882, 1280, 2400 and 4800 with 16, 2 and 1 frames per chunk, two layouts above 64 KiB of LDS (4800 points; 4410 lags direct), 1, 15, 16 and 17 frames around a workgroup's run,
three lead shapes, both precisions, uncentred, every pad mode, min_period 2, thresholds 0, 0.1 and 1, the first and the last lag.

Measured on the MI355X (printed per case): no settled frame at another lag than the reference's; worst f0 error 1.3e-15 relative (case thr1,
bound 6.7e-15), at most 0.28 of the case's bound everywhere; float64 CMND within 5.5e-15 of the model (bounds 1.4e-14 .. 6.4e-14); float32 CMND
within 5.94e-8, which is its one rounding to float32 (bound 5.96e-8), and never further from the model than twice the reference's float32 run."""
import warnings

import numpy as np
import pytest

import librosa_amd as L
import yin_cases as YC
from librosa_amd.core import pitch as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return YC.load()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _quiet(fn):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn()


@pytest.mark.parametrize("name", list(YC.CASES))
def test_yin_matches_the_reference(golden, name):
    z, meta = golden
    y, kw = YC.signal(name), YC.CASES[name]["kw"]
    assert YC.digest(y) == meta["cases"][name]["y"]
    before = y.copy()
    got = _quiet(lambda: L.yin(y, **kw))
    assert isinstance(got, np.ndarray) and np.array_equal(y, before)
    YC.check_f0(got, name, z, meta)


FRAMES_CASES = ["w64_glide", "w512_gap", "w512_glide64", "w1001_gap64", "w2048_glide", "w4500_gap64", "frames17", "lead2", "nocenter", "reflect", "nyquist", "last_lag",
                "two_periods_warning", "w2048_fmin11", "w8192_fmin5"]


@pytest.mark.parametrize("name", FRAMES_CASES)
def test_yin_frames_match_the_reference(golden, name):
    z, meta = golden
    y, kw = YC.signal(name), dict(YC.CASES[name]["kw"])
    kw.pop("trough_threshold", None)
    cm, sh, p0 = _quiet(lambda: P._yin_frames(y, **kw))
    want = z["cmnd_" + name]
    assert isinstance(cm, np.ndarray) and cm.dtype == sh.dtype == y.dtype and cm.shape == sh.shape == want.shape and p0 == YC.periods(kw)[0]
    YC.check_frames(cm, sh, YC.model64(name), want, meta["cases"][name], y.dtype)


@pytest.mark.parametrize("name", ["w512_gap", "w2048_noise64", "w4500_glide", "lead2", "reflect"])
def test_device_tensor_gives_the_bits_of_the_numpy_call(name):
    import torch

    y, kw = YC.signal(name), YC.CASES[name]["kw"]
    host = L.yin(y, **kw)
    t = _dev(y)
    keep = t.clone()
    got = L.yin(t, **kw)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == host.shape
    assert np.array_equal(got.cpu().numpy(), host)
    assert torch.equal(t, keep), "the input was written"
    kw = {k: v for k, v in kw.items() if k != "trough_threshold"}
    cm, sh, _ = P._yin_frames(t, **kw)
    hcm, hsh, _ = P._yin_frames(y, **kw)
    assert cm.is_cuda and sh.is_cuda and np.array_equal(cm.cpu().numpy(), hcm) and np.array_equal(sh.cpu().numpy(), hsh)
    assert torch.equal(t, keep), "the input was written"


def test_a_clip_gives_the_same_bits_alone_and_in_a_batch():
    for name in ("lead2", "lead2_64"):
        y, kw = YC.signal(name), YC.CASES[name]["kw"]
        whole = L.yin(y, **kw)
        assert np.array_equal(whole[1, 2], L.yin(y[1, 2], **kw)) and np.array_equal(whole[0], L.yin(y[0], **kw))


def test_host_pad_modes_are_refused_for_device_tensors():
    y, kw = YC.signal("linear_ramp64"), YC.CASES["linear_ramp64"]["kw"]
    with pytest.raises(L.ParameterError):
        L.yin(_dev(y), **kw)
