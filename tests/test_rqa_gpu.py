"""sequence.rqa on the MI355X against tests/golden/rqa.npz (the unmodified reference), under the rule of tests/rqa_cases.py: ``score`` bit-equal
(the hash, the stored row and column), ``path`` equal -- for the two quirk cases, whose reference walk leaves the matrix through column 1, equal to
the walk along the moves that were scored.

Shapes are the smallest at which the kernels can go wrong (tests/rqa_cases.py): 1 x 1, 1 x 7, 7 x 1, 2 x 2, 2 x 9, 9 x 2 and 3 x 3 for the init
paths; blocks and strips forced to (1, 4) at 9 x 14, (4, 8) at 20 x 37 and 37 x 20, (8, 16) at 33 x 70 and (16, 16) at 40 x 50, where the halo
spans two strips; the shipped geometry at shapes two over it and three over twice it.  Inputs: sparse weighted, binary (exact ties), dense, all
zeros, negative entries, NaN; seven gap settings with knight moves on and off; float32; bool, uint8, int32, int64 and int16."""
import numpy as np
import pytest

import librosa_amd as L  # noqa: F401
import rqa_cases as RC
from librosa_amd import sequence as S

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", list(RC.CASES))
def test_numpy_call_matches_the_reference(name):
    score, path = RC.run_case(name, S)
    assert isinstance(score, np.ndarray) and isinstance(path, np.ndarray)
    RC.check_case(name, score, path)


@pytest.mark.parametrize("name", [n for n, c in RC.CASES.items() if c["rows"] and c["kind"] in ("binary", "sparse") and c["dtype"] == "float64"])
def test_forced_geometry_equals_the_default_geometry(name):
    for a, b in zip(RC.run_case(name, S), RC.run_case(name, S, geometry=(0, 0))):
        assert np.array_equal(a, b, equal_nan=True)


_big = {}


def big():
    """257 x 300 binary (every tie exact) and what the model makes of it, computed once."""
    if not _big:
        sim = (np.random.default_rng(4343).random((257, 300)) < 0.3).astype(np.float64)
        _big["sim"] = sim
        for kw in (dict(), dict(gap_onset=np.inf, gap_extend=np.inf, knight_moves=False)):
            _big[tuple(kw)] = RC.model_rqa(sim, **kw)
    return _big


@pytest.mark.parametrize("geometry", [(0, 0), (4, 8), (16, 16)])
@pytest.mark.parametrize("kw", [dict(), dict(gap_onset=np.inf, gap_extend=np.inf, knight_moves=False)], ids=["q_knight", "l_mode"])
def test_many_launches_and_strips_equal_the_model(geometry, kw):
    # 5 launches of 5 strips at the default geometry, 65 launches of 38 strips at (4, 8), 17 of 19 at (16, 16)
    m_score, m_path, _ = big()[tuple(kw)]
    score, path = RC.run(S, big()["sim"], *geometry, **kw)
    assert np.array_equal(score, m_score) and np.array_equal(path, m_path) and path.dtype == np.uint64


TENSOR_CASES = [n for n, c in RC.CASES.items()
                if (c["rows"], c["strip"]) in ((16, 16), (1, 4)) and c["gaps"] in ((1, 1), (RC.INF, RC.INF), (0.3, 0.7)) or c["dtype"] in ("bool", "uint8", "int32", "int64") and c["N"] == 20
                or n in RC.QUIRKS or (c["N"], c["M"]) == (1, 1) and c["gaps"] == (1, 1)]


@pytest.mark.parametrize("name", TENSOR_CASES)
def test_device_tensor_gives_the_bits_of_the_numpy_call(name):
    import torch

    host = RC.run_case(name, S)
    kept = []

    def wrap(a):
        kept.append((_dev(a), _dev(a)))
        return kept[-1][0]

    score, path = RC.run_case(name, S, wrap=wrap)
    for t, h in ((score, host[0]), (path, host[1])):
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == getattr(torch, h.dtype.name) and tuple(t.shape) == h.shape
        assert np.array_equal(t.cpu().numpy().view(f"u{h.itemsize}"), h.view(f"u{h.itemsize}"))
    for given, copy in kept:
        assert np.array_equal(given.cpu().numpy(), copy.cpu().numpy(), equal_nan=given.dtype.is_floating_point), "the input was written"


def test_backtrack_false_returns_score_alone():
    import torch

    sim = RC.inputs(next(n for n, c in RC.CASES.items() if c["kind"] == "sparse" and (c["N"], c["M"]) == (33, 70)))
    score, path = S.rqa(sim)
    only = S.rqa(sim, backtrack=False)
    assert isinstance(only, np.ndarray) and np.array_equal(only, score) and len(path) > 0
    only = S.rqa(_dev(sim), backtrack=False)
    assert isinstance(only, torch.Tensor) and only.is_cuda and np.array_equal(only.cpu().numpy(), score)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.uint8])
def test_the_empty_path_has_shape_0_2_and_the_right_dtype(dtype):
    import torch

    score, path = S.rqa(np.zeros((40, 50), dtype=dtype))
    assert path.shape == (0, 2) and path.dtype == np.uint64 and score.dtype == (dtype if dtype != np.uint8 else np.float64) and not score.any()
    score, path = S.rqa(_dev(np.zeros((40, 50), dtype=dtype)))
    assert tuple(path.shape) == (0, 2) and path.dtype == torch.uint64 and path.is_cuda and not bool(score.any())
