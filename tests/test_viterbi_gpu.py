"""sequence.viterbi, viterbi_discriminative, viterbi_binary and _viterbi_log on the MI355X against tests/golden/viterbi.npz (the unmodified
reference), under the two rules of tests/viterbi_cases.py: log-domain cases bit-equal in states and logp; public-path cases at the reference's
states with logp within delta = T (4 * 2^-52 * 709 + 2 ulp(|logp|)) (delta32 = T (2 * 2^-24 * 88 + 2 ulp(|logp|)) for the float32 case).

Shapes are the smallest at which the kernels can go wrong (tests/viterbi_cases.py): 1, 2, 3, 31, 32, 33 (the small kernel's boundary), 63, 64,
65 (the lane splits), 257 and 1025 states (several targets per thread), full and thresholded; 1, 2, 31, 32 and 33 steps around the prepare
kernel's tile; lead shapes (), (3,), (2, 3) and 130 two-state chains (more than a workgroup of the small kernel holds); pyin's transition at 242
x 40 and 1200 x 5 with 1e-4; p_init and p_state given and default; viterbi_binary with one shared and with per-label tables, 5 and 70 labels; one
float32 case; 8192 states through a band; uniform, exact ties, probability zeros and a target without a finite candidate in the log domain.

Measured on the MI355X (printed per case): every log-domain case bit-equal; every public-path case at the reference's states; worst logp error
1.78e-15 for float64 prob (case v_many, bound 3.79e-12; b_tables70 8.9e-16, every other case 0) and 1.37e-06 for the float32 case (bound 4.2e-04)."""
import numpy as np
import pytest

import librosa_amd as L
import viterbi_cases as VC
from librosa_amd import sequence as S

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", list(VC.CASES))
def test_numpy_call_matches_the_reference(name):
    states, logp = VC.run_case(name, S)
    assert isinstance(states, np.ndarray) and isinstance(logp, np.ndarray)
    VC.check_case(name, states, logp, report=print)


TENSOR_CASES = ["v_s3", "d_s33_thr", "d_s257_thr", "v_lead3", "d_lead23", "v_many", "pyin_242", "b_shared5", "b_tables70", "b_1d", "v_f32", "d_t33", "log_ties_split", "log_neginf_small",
                "log_ties_small"]


@pytest.mark.parametrize("name", TENSOR_CASES)
def test_device_tensor_gives_the_bits_of_the_numpy_call(name):
    import torch

    host = VC.run_case(name, S)
    kept = []

    def wrap(a):
        kept.append((_dev(a), _dev(a)))
        return kept[-1][0]

    states, logp = VC.run_case(name, S, wrap=wrap)
    assert isinstance(states, torch.Tensor) and states.is_cuda and states.dtype == torch.uint16 and tuple(states.shape) == host[0].shape
    assert isinstance(logp, torch.Tensor) and logp.is_cuda and logp.dtype == torch.float64 and tuple(logp.shape) == host[1].shape
    assert np.array_equal(states.cpu().numpy(), host[0]) and np.array_equal(logp.cpu().numpy(), host[1], equal_nan=True)
    assert torch.equal(kept[0][0], kept[0][1]), "the input was written"


def test_states_alone_are_returned_without_return_logp():
    a = VC.inputs("v_s3")
    states = S.viterbi(a["prob"], a["transition"], **a["kw"])
    assert isinstance(states, np.ndarray) and np.array_equal(states, VC.load()[0]["v_s3/states"])
    b = VC.inputs("b_shared5")
    assert np.array_equal(S.viterbi_binary(b["prob"], b["transition"], **b["kw"]), VC.load()[0]["b_shared5/states"])


@pytest.mark.parametrize("name", ["d_lead23", "v_lead23_thr", "v_many", "b_tables70", "log_ties_small"])
def test_batch_equals_per_item_bit_for_bit(name, monkeypatch):
    c, a = VC.CASES[name], VC.inputs(name)
    whole = VC.run_case(name, S)
    if c["fn"] == "log":
        items = [S._viterbi_log(x, a["log_trans"], a["log_p_init"], a["thr"]) for x in a["log_prob"]]
    else:
        items = [VC.functions(S)[c["fn"]](x, a["transition"], return_logp=True, **a["kw"]) for x in a["prob"].reshape((-1,) + a["prob"].shape[len(c["lead"]):])]
    assert np.array_equal(np.stack([i[0] for i in items]).reshape(whole[0].shape), whole[0])
    assert np.array_equal(np.stack([i[1] for i in items]).reshape(whole[1].shape), whole[1])
    # a scratch budget of two sequences (binary: of one item's labels): several launches, the same bits
    monkeypatch.setattr(S, "SCRATCH_BUDGET", 10 * 2 * c["T"] * c["S"])
    chunked = VC.run_case(name, S)
    assert np.array_equal(chunked[0], whole[0]) and np.array_equal(chunked[1], whole[1])


@pytest.mark.parametrize("name", [n for n, r in VC.refusals().items() if r[4]])
def test_prob_range_is_refused_with_the_reference_text(name):
    fn, prob, transition, kw, _ = VC.refusals()[name]
    with pytest.raises(L.ParameterError) as e:
        getattr(S, fn)(prob, transition, **kw)
    assert str(e.value) == VC.load()[1]["refusals"][name]
    with pytest.raises(L.ParameterError) as e:
        getattr(S, fn)(_dev(prob), transition, **kw)
    assert str(e.value) == VC.load()[1]["refusals"][name]
