"""pyin on the MI355X: parts (a) to (d) of tests/pyin_cases.py against tests/golden/pyin.npz (the unmodified reference).

(a) the observation kernel alone on the reference's own float64 CMND, against ``__pyin_helper``: zero probabilities store log(tiny) bit for bit,
    a voiced entry within (n_thresholds + 8) 2^-52 + 2 ulp of log(p_ref + tiny), voiced_prob within (n_thresholds + n_lags) 2^-52, an unvoiced
    probability within 2 * that / P + 4 * 2^-52 u_ref; derived bounds, every candidate's bin more than 1e-9 from a rounding half.
(b) pyin against the NumPy Viterbi model run on the device's own table: voiced_flag and f0 bit for bit, fill_na None / nan / 0.0, at 24, 50, 242
    and 1202 states, thresholded and (24, 50) full search.
(c) pyin against the reference's pyin on certified clips of at most 0.5 s: voiced_prob within the bound of (a), voiced_flag and f0 equal; up to
    242 states the device path's score under the reference's tables at least the reference path's minus 2 T 1e-10.
(d) the refusals.

Shapes: 130 lags (two rounds of 64 and a tail of 2), 1 / 63 / 64 / 65 frames around the four-frame workgroup, 1 / 100 / 130 thresholds around the
64 lanes, more than 64 troughs in a frame, lead shapes () and (2, 3).

Measured on the MI355X (printed per case), the simulator's figures bit for bit: (a) worst voiced entry 7.1e-15 from log(p_ref + tiny) (0.19 of its
bound), voiced_prob 2.2e-16 (bound 5.1e-14), an unvoiced probability 6.9e-18 off (0.005 of its bound); (b) every case bit-equal; (c) voiced_prob
within 2.2e-16 (bounds 3.1e-14 and 9.5e-14), voiced_flag and f0 equal everywhere, score gap 0 in every case of at most 242 states."""
import numpy as np
import pytest

import librosa_amd as L
import pyin_cases as PC
from librosa_amd import sequence as S
from librosa_amd.core import pitch as P

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def golden():
    return PC.load()


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.OBS_CASES))
def test_observation_kernel_matches_the_reference(golden, name):
    PC.run_obs_case(name, P, golden[0], report=print)


@pytest.mark.parametrize("name", ["syn", "noise_lead23", "noise_thr130"])
def test_observation_kernel_on_device_tensors(golden, name):
    import torch

    kw = PC.obs_kw(name)
    p = PC.obs_params(kw)[0]
    cm, sh = PC.obs_inputs(name, golden[0])
    host = P._pyin_log_prob(cm, sh, **p)
    a, b = _dev(cm), _dev(sh)
    log_prob, vp = P._pyin_log_prob(a, b, **p)
    assert isinstance(log_prob, torch.Tensor) and log_prob.is_cuda and log_prob.dtype == vp.dtype == torch.float64
    assert np.array_equal(log_prob.cpu().numpy(), host[0]) and np.array_equal(vp.cpu().numpy(), host[1])
    assert torch.equal(a, _dev(cm)) and torch.equal(b, _dev(sh)), "the inputs were written"
    PC.run_obs_case(name, P, golden[0], wrap=_dev)


def test_a_clip_gives_the_same_bits_alone_and_in_a_batch(golden):
    cm, sh = PC.obs_inputs("noise_lead23", golden[0])
    p = PC.obs_params(PC.obs_kw("noise_lead23"))[0]
    whole = P._pyin_log_prob(cm, sh, **p)
    one = P._pyin_log_prob(cm[1, 2], sh[1, 2], **p)
    assert np.array_equal(whole[0][1, 2], one[0]) and np.array_equal(whole[1][1, 2], one[1])


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tmp", [(n, t) for n, c in PC.GLUE_CASES.items() for t in ((1e-4, None) if c["none"] else (1e-4,))])
def test_decode_glue_is_exact(name, tmp):
    voiced, frames = PC.run_glue_case(name, L, tmp)
    assert 0 < voiced < frames


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.E2E_CASES))
def test_pyin_matches_the_reference(golden, name):
    out = PC.run_e2e_case(name, L, golden[0], report=print)
    assert all(isinstance(o, np.ndarray) for o in out)
    if "eobs_" + name in golden[0]:
        print(name, "score gap", PC.check_e2e_score(name, L, golden[0]))


def test_float32_input_equals_its_float64_cast(golden):
    y = PC.e2e_signal("e_f32")
    assert y.dtype == np.float32
    a, b = L.pyin(y, **PC.E2E_CASES["e_f32"]["kw"]), L.pyin(y.astype(np.float64), **PC.E2E_CASES["e_f32"]["kw"])
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and np.array_equal(u, v, equal_nan=True)


def test_batch_device_tensor_and_chunks_give_the_same_bits(golden, monkeypatch):
    import torch

    c = PC.E2E_CASES["e_lead23"]
    y = PC.e2e_signal("e_lead23")
    whole = L.pyin(y, **c["kw"])
    one = L.pyin(y[1, 2], **c["kw"])
    t = _dev(y)
    dev = L.pyin(t, **c["kw"])
    assert all(isinstance(d, torch.Tensor) and d.is_cuda for d in dev) and [d.dtype for d in dev] == [torch.float64, torch.bool, torch.float64]
    assert torch.equal(t, _dev(y)), "y was written"
    n_lags, n_frames = 74 - 36 + 1, whole[0].shape[-1]
    monkeypatch.setattr(S, "SCRATCH_BUDGET", 2 * (16 * n_lags + 10 * 242) * n_frames)   # two clips per chunk: three chunks
    chunked = L.pyin(y, **c["kw"])
    chunked_dev = L.pyin(t, **c["kw"])
    for a, o, d, ch, chd in zip(whole, one, dev, chunked, chunked_dev):
        assert np.array_equal(a[1, 2], o, equal_nan=True)
        assert np.array_equal(a, d.cpu().numpy(), equal_nan=True) and tuple(d.shape) == a.shape
        assert np.array_equal(a, ch, equal_nan=True) and np.array_equal(a, chd.cpu().numpy(), equal_nan=True)


def test_an_empty_batch_gives_empty_results():
    import torch

    kw = PC.E2E_CASES["e_noise"]["kw"]
    n_frames = 1 + 1000 // 64
    for y in (np.zeros((0, 1000)), torch.zeros((0, 1000), dtype=torch.float64, device="cuda")):
        f0, flag, vp = L.pyin(y, **kw)
        assert tuple(f0.shape) == tuple(flag.shape) == tuple(vp.shape) == (0, n_frames) and type(f0) is type(y)


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.refusal_calls()))
def test_refusals(golden, name):
    PC.check_refusal(name, L, golden[1])
