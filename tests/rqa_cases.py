"""Cases, inputs and the NumPy model of ``sequence.rqa``, shared by ``scripts/make_rqa_golden.py``, ``tests/test_rqa_host.py`` and
``tests/test_rqa_gpu.py``.

TEST INFRASTRUCTURE ONLY.  Inputs come from seeds.  ``tests/golden/rqa.npz`` holds, per case, what the unmodified reference returns: ``path``,
the last row and the last column of ``score``, the SHA-256 of the bytes of ``score``, and whether the reference's walk left the matrix; and the
two refusal texts.

The model (``model``) is the recurrence run one row at a time, written from its rules: row 0 and column 0 copy ``sim`` (pointer -2 where it is
non-zero, else -1); cell (i, j) takes the diagonal, with knight moves the left knight (i-1, j-2) if j >= 2 and the up knight (i-2, j-1) if
i >= 2, in that order; ``s_c`` is the candidate's stored score widened to float64, ``t_c = sim[candidate] > 0``; where ``sim[i, j] > 0`` the score
is ``s_k + sim[i, j]`` for ``k = argmax(s)``, else ``v_c = (s_c - t_c * gap_onset) - (~t_c) * gap_extend``, ``k = argmax(v)`` and the score is
``v_k`` if that is positive, else +0.0 (pointer -1 where the stored score is zero).  ``argmax`` is NumPy's: the first maximum, a NaN first.  The
pointers are the device's codes (0 diagonal, 1 left knight, 2 up knight): they name the move.  The reference numbers the candidates of a cell in
the order they exist, so in column 1 its code for the up knight is 1, which its walk reads as the left knight: ``walk(..., reference=True)`` reads
the pointers that way, Python's negative indices included, and says whether the walk left the matrix.  The generator asserts that the model
reproduces the reference's ``score`` bit for bit on every case and its ``path`` on every case whose walk stays inside.

One rule: ``score`` is bit-equal to the golden (the hash and the stored row and column; a mismatch is localised with the model) and ``path`` is
equal to the golden's -- for the two quirk cases, whose reference walk leaves the matrix, to the model's walk along the moves that were scored.
bool and integer ``sim`` are judged against the reference on ``sim.astype(float64)``.
"""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rqa.npz")
DEFAULT_ROWS, DEFAULT_STRIP = 64, 64    # csrc/lra_rqa.h: kDefaultRows, kDefaultStrip
INF = float("inf")
GAPS = [(1, 1), (5, 10), (0.3, 0.7), (0, 0), (INF, INF), (INF, 0.5), (0.5, INF)]
KINDS = ["sparse", "binary", "dense", "zeros", "neg", "nan"]
INIT_SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (2, 9), (9, 2), (3, 3)]
# (rows, strip, N, M): forced geometries (many launches and strips at tiny shapes; at (16, 16) the halo of 30 spans two strips), and the shipped
# defaults (0, 0) at shapes that straddle them
FORCED = [(1, 4, 9, 14), (4, 8, 20, 37), (4, 8, 37, 20), (8, 16, 33, 70), (16, 16, 40, 50)]
SHIPPED = [(0, 0, DEFAULT_ROWS + 2, DEFAULT_STRIP + 2), (0, 0, 2 * DEFAULT_ROWS + 3, 2 * DEFAULT_STRIP + 3)]

# name -> dict(N, M, kind, gaps, knight, rows, strip, dtype, seed)
CASES = {}
# cases whose first seed led the reference's walk out of the matrix through column 1 (the generator refuses those): name -> the seed that stays inside
RESEED = {
    "9x2_dense_5_10_k_float64": 13072,
    "9x2_sparse_0_0_k_float64": 11076,
    "9x2_dense_inf_inf_k_float64": 16078,
    "9x2_sparse_0p5_inf_k_float64": 10082,
    "37x20_dense_0p3_0p7_k_float64_r4w8": 13130,
    "37x20_neg_0_0_k_float64_r4w8": 10132,
    "37x20_sparse_inf_inf_k_float64_r4w8": 10134,
    "37x20_dense_inf_0p5_k_float64_r4w8": 11136,
    "66x66_binary_0_0_k_float64": 10174,
    "37x20_dense_1_1_k_float64_r4w8": 10220,
    "40x50_binary_1_1_k_float32_r16w16": 10291,
    "3x3_sparse_0p3_0p7_k_float32": 10308,
}


def _gap_word(g):
    return "inf" if g == INF else str(g).replace(".", "p")


def _add(N, M, kind, gaps, knight, rows=0, strip=0, dtype="float64", seed=None, tag=""):
    name = f"{tag}{N}x{M}_{kind}_{_gap_word(gaps[0])}_{_gap_word(gaps[1])}_{'k' if knight else 'd'}_{dtype}" + (f"_r{rows}w{strip}" if rows else "")
    if name not in CASES:
        CASES[name] = dict(N=int(N), M=int(M), kind=kind, gaps=gaps, knight=bool(knight), rows=int(rows), strip=int(strip), dtype=dtype, seed=RESEED.get(name, 9000 + len(CASES)) if seed is None else seed)
    return name


# every shape and geometry with every gap setting, knight moves on and off, the kind of input rotating through them
for _g, (_r, _w, _N, _M) in enumerate([(0, 0, n, m) for n, m in INIT_SHAPES] + FORCED + SHIPPED):
    for _k, _gaps in enumerate(GAPS):
        for _knight in (True, False):
            _add(_N, _M, KINDS[(_g + 2 * _k + int(_knight)) % len(KINDS)], _gaps, _knight, _r, _w)
# every kind of input at every geometry that has more than one launch or strip: the default gaps with knight moves, and L mode
for _r, _w, _N, _M in FORCED + SHIPPED:
    for _kind in KINDS:
        _add(_N, _M, _kind, (1, 1), True, _r, _w)
        _add(_N, _M, _kind, (INF, INF), False, _r, _w)
# float32: scored in its own type (0.3 and 0.7 are inexact, the sums round on the store)
for _r, _w, _N, _M in FORCED + SHIPPED[:1]:
    for _kind, _gaps, _knight in (("sparse", (0.3, 0.7), True), ("binary", (1, 1), True), ("dense", (5, 10), False), ("neg", (INF, 0.5), True), ("nan", (0.5, INF), True), ("zeros", (1, 1), True)):
        _add(_N, _M, _kind, _gaps, _knight, _r, _w, dtype="float32")
for _N, _M in INIT_SHAPES:
    _add(_N, _M, "sparse", (0.3, 0.7), True, dtype="float32")
# bool and integers: widened exactly, judged against the reference on astype(float64); int16 takes the cast
for _dtype in ("bool", "uint8", "int32", "int64", "int16"):
    _add(20, 37, "ints", (1, 1), True, 4, 8, dtype=_dtype)
    _add(20, 37, "ints", (0.3, 0.7), False, 4, 8, dtype=_dtype)
    _add(3, 3, "ints", (1, 1), True, dtype=_dtype)
# the reference's walk leaves the matrix through column 1: the expected path is the model's
QUIRKS = [_add(6, 6, "quirk_a", (1, 1), True, tag="q_"), _add(6, 6, "quirk_b", (1, 1), True, tag="q_")]


def inputs(name):
    """``sim`` of a case."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    N, M, kind = c["N"], c["M"], c["kind"]
    values, mask = rng.random((N, M)), rng.random((N, M)) < 0.3
    if kind == "sparse":
        sim = values * mask
    elif kind == "binary":
        sim = mask.astype(np.float64)
    elif kind == "dense":
        sim = values + 0.01
    elif kind == "zeros":
        sim = np.zeros((N, M))
    elif kind == "neg":   # negative entries in the first row, the first column and the interior
        sim = values * mask
        sim[rng.random((N, M)) < 0.15] *= -1.0
        sim[0, M // 2] = sim[N // 2, 0] = sim[N // 2, M // 2] = -0.5
    elif kind == "nan":   # a NaN in row 0 and one in the interior
        sim = values * mask
        sim[0, min(1, M - 1)] = np.nan
        sim[N // 2, M // 2] = np.nan
    elif kind == "ints":
        sim = (rng.integers(0, 4, size=(N, M)) * mask).astype(np.float64)
        if c["dtype"] == "bool":
            sim = mask
    elif kind in ("quirk_a", "quirk_b"):
        sim = np.zeros((6, 6))
        sim[0, 0] = sim[2, 1] = sim[3, 2] = sim[4, 3] = 1.0
        if kind == "quirk_b":
            sim[1, 5] = 1.0
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(sim.astype(c["dtype"]))


def kwargs(name):
    c = CASES[name]
    return dict(gap_onset=c["gaps"][0], gap_extend=c["gaps"][1], knight_moves=c["knight"])


def geometry(name):
    """(rows, strip) a case runs under."""
    c = CASES[name]
    return (c["rows"] or DEFAULT_ROWS, c["strip"] or DEFAULT_STRIP)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
def model(sim, gap_onset=1, gap_extend=1, knight_moves=True):
    """``score`` (sim's type; float64 for bool and integers) and the device's pointers (int8), one row at a time."""
    sim = np.asarray(sim)
    if sim.dtype.kind in "biu":
        sim = sim.astype(np.float64)
    N, M = sim.shape
    score = np.zeros((N, M), dtype=sim.dtype)
    ptr = np.zeros((N, M), dtype=np.int8)
    score[0, :], score[:, 0] = sim[0, :], sim[:, 0]
    ptr[0, :] = np.where(sim[0, :] != 0, -2, -1)
    ptr[:, 0] = np.where(sim[:, 0] != 0, -2, -1)
    pos = sim > 0
    go, ge = np.float64(gap_onset), np.float64(gap_extend)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(1, N):
            if M < 2:
                break
            s, t, have = np.zeros((3, M - 1)), np.zeros((3, M - 1), dtype=bool), np.zeros((3, M - 1), dtype=bool)
            s[0], t[0], have[0] = score[i - 1, :M - 1], pos[i - 1, :M - 1], True
            if knight_moves:
                s[1, 1:], t[1, 1:], have[1, 1:] = score[i - 1, :M - 2], pos[i - 1, :M - 2], True
                if i >= 2:
                    s[2], t[2], have[2] = score[i - 2, :M - 1], pos[i - 2, :M - 1], True
            v = s - t * go
            v = v - (~t) * ge
            hit = pos[i, 1:]
            val = np.where(hit, s, v)
            best, k = val[0].copy(), np.zeros(M - 1, dtype=np.int8)
            for c in (1, 2):
                take = have[c] & ~np.isnan(best) & (np.isnan(val[c]) | (val[c] > best))
                best, k = np.where(take, val[c], best), np.where(take, c, k).astype(np.int8)
            out_hit = (best + sim[i, 1:].astype(np.float64)).astype(sim.dtype)
            out_gap = np.where(best > 0, best, 0.0).astype(sim.dtype)
            score[i, 1:] = np.where(hit, out_hit, out_gap)
            ptr[i, 1:] = np.where(hit | (out_gap != 0), k, -1)
    return score, ptr


MOVES = [(-1, -1), (-1, -2), (-2, -1)]


def walk(score, ptr, reference=False):
    """The path (uint64, (k, 2)) from ``np.argmax(score)`` along the pointers.  ``reference``: as the reference reads them -- the up knight of
    column 1 carries its code 1, the left knight's, and an index below zero wraps as Python's does; then also whether the walk left the matrix."""
    N, M = score.shape
    i, j = (int(x) for x in np.unravel_index(np.argmax(score), score.shape))
    path, left = [], False
    while len(path) <= N + M:
        code = int(ptr[i, j])   # (a negative index wraps here as it does in the reference)
        if reference and code == 2 and j % M == 1:
            code = 1
        if code == -1:
            break
        path.insert(0, (i, j))
        if code == -2:
            break
        i, j = i + MOVES[code][0], j + MOVES[code][1]
        if i < 0 or j < 0:
            left = True
            if not reference or i < -N or j < -M:
                break
    out = np.asarray([(a % 2**64, b % 2**64) for a, b in path], dtype=np.uint64).reshape(-1, 2)
    return (out, left) if reference else out


def model_rqa(sim, **kw):
    """What ``rqa(sim, **kw)`` returns, by the model: (score, path, pointers)."""
    score, ptr = model(sim, **kw)
    return score, walk(score, ptr), ptr


def refusals():
    """name -> kwargs the reference refuses with a ParameterError whose text the golden holds."""
    return {"gap_onset": dict(gap_onset=-1.0), "gap_extend": dict(gap_extend=-0.5), "both": dict(gap_onset=-2, gap_extend=-2)}


def limits():
    """name -> (sim, a word of the message): the documented differences, refused before any device work."""
    return {
        "complex": (np.ones((3, 4), dtype=np.complex64), "real-valued"),
        "strings": (np.array([["a", "b"], ["c", "d"]]), "real-valued"),
        "objects": (np.array([[None, 1], [2, 3]], dtype=object), "real-valued"),
        "one_dimension": (np.ones(5), "must be a matrix"),
        "three_dimensions": (np.ones((2, 3, 4)), "must be a matrix"),
        "no_rows": (np.ones((0, 4)), "empty"),
        "no_columns": (np.ones((4, 0)), "empty"),
    }


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


_golden = None


def load():
    """(arrays, meta) of tests/golden/rqa.npz."""
    global _golden
    if _golden is None:
        z = np.load(GOLDEN)
        _golden = ({k: z[k] for k in z.files if k != "meta"}, json.loads(str(z["meta"])))
    return _golden


# ---- running and judging a case (host simulator and device alike) --------------------------------------------------------------------------------
def run(seq, sim, rows, strip, **kw):
    old = seq.RQA_ROWS, seq.RQA_STRIP
    seq.RQA_ROWS, seq.RQA_STRIP = rows, strip
    try:
        return seq.rqa(sim, **kw)
    finally:
        seq.RQA_ROWS, seq.RQA_STRIP = old


def run_case(name, seq, wrap=lambda a: a, geometry=None, **more):
    """A case through the package (seq: librosa_amd.sequence; wrap: what turns ``sim`` into the caller's kind of array): (score, path) as
    returned.  geometry: (rows, strip), the case's own unless given."""
    c, sim = CASES[name], inputs(name)
    before = sim.copy()
    rows, strip = (c["rows"], c["strip"]) if geometry is None else geometry
    out = run(seq, wrap(sim), rows, strip, **kwargs(name), **more)
    assert np.array_equal(before, sim, equal_nan=sim.dtype.kind == "f"), "the input was written"
    return out


def expected_dtype(name):
    dtype = np.dtype(CASES[name]["dtype"])
    return dtype if dtype.kind == "f" else np.dtype(np.float64)


def _first_difference(name, score):
    m_score = model(inputs(name), **kwargs(name))[0]
    bad = np.argwhere(score.view(f"u{score.itemsize}") != m_score.view(f"u{score.itemsize}"))
    if not len(bad):
        return "equal to the model"
    i, j = bad[0]
    return f"first cell off the model: ({i}, {j}): {score[i, j]!r} against {m_score[i, j]!r}; {len(bad)} cells differ"


def check_case(name, score, path):
    """The rule of rqa_cases against the golden."""
    arrays, meta = load()
    entry = meta["cases"][name]
    c = CASES[name]
    assert score.dtype == expected_dtype(name) and score.shape == (c["N"], c["M"])
    assert path.dtype == np.uint64 and path.ndim == 2 and path.shape[1] == 2
    assert sha(score) == entry["sha_score"], f"{name}: score is not bit-equal to the reference's; {_first_difference(name, score)}"
    assert np.array_equal(score[-1], arrays[f"{name}/row"], equal_nan=True) and np.array_equal(score[:, -1], arrays[f"{name}/col"], equal_nan=True)
    want = model_rqa(inputs(name), **kwargs(name))[1] if entry["left"] else arrays[f"{name}/path"]
    assert np.array_equal(path, want), f"{name}: path {path.tolist()} against {want.tolist()}"
