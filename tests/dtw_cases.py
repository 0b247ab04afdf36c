"""Cases, inputs and the NumPy model of ``sequence.dtw`` and ``sequence.dtw_backtracking``, shared by ``scripts/make_dtw_golden.py``,
``tests/test_dtw_host.py`` and ``tests/test_dtw_gpu.py``.

TEST INFRASTRUCTURE ONLY.  Inputs come from seeds.  ``tests/golden/dtw.npz`` holds, per case, what the unmodified reference returns: ``wp``, the
last row and the last column of ``D``, the SHA-256 of the bytes of ``D`` and of ``steps``; the messages of the refused calls; and per X/Y case
its margin and ``delta``.

The model (``model``) is the reference's recurrence run one anti-diagonal at a time: every cell of an anti-diagonal takes its candidates in step
order, each ``cur_C = w_mul * C; cur_C += w_add; cost = D_prev + cur_C`` in float64 and a strict ``<``.  The generator asserts that it reproduces
the reference's ``D``, ``steps`` and ``wp`` bit for bit on every case.

Two rules.
  * ``C=`` path and ``dtw_backtracking``: ``D``, ``steps`` and ``wp`` are bit-equal to the golden (the hashes and the stored rows; a mismatch is
    localised with the model).
  * ``X, Y`` path: the device forms the cost matrix itself and is not promised scipy's bits.  ``eps_C`` bounds how far two correctly rounded
    float64 evaluations of a metric over K features of magnitude up to R can lie apart, whatever their order of summation (u = 2**-53; a sum of K
    non-negative terms carries a relative error of at most (K - 1) u, each term of at most 2 u):
        sqeuclidean  2 (K + 2) u K (2R)^2
        euclidean    2 (K + 3) u sqrt(K) 2R            (the root halves the relative error of the sum and rounds once more)
        cityblock    2 (K + 1) u K 2R
        cosine       2 (2K + 8) u                       (the dot product and both norms against |x||y|, the product, the quotient, 1 - c)
    No cell of ``D`` then moves further than ``delta = (N + M - 1) (max|w_mul| eps_C + 3 ulp(max finite D))``: a path has at most N + M - 1 cells
    and each adds one cost and rounds three times at most at the size of the running value.  A case is CERTIFIED when the smallest gap between the
    chosen and the next candidate over the cells of the reference's path and, under ``subseq``, the gap of the final argmin are at least
    ``MARGIN_FLOOR`` and at least ``MARGIN_FACTOR * delta``; then ``wp`` is equal and ``D`` is within ``delta``.  Every X/Y case must certify; one
    that does not gets another seed.
"""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "dtw.npz")
MARGIN_FLOOR, MARGIN_FACTOR = 1e-6, 4.0
MAX_STEPS, MAX_STEP = 16, 8     # csrc/lra_dtw.h: kMaxSteps, kMaxStep
DEFAULT_TILE = 64               # kDefaultTile
DEFAULT_STEPS = np.array([[1, 1], [0, 1], [1, 0]])
METRICS = ("euclidean", "sqeuclidean", "cityblock", "cosine")
STEPS_16 = [[1, 1], [1, 2], [2, 1], [2, 2], [1, 3], [3, 1], [2, 3], [3, 2], [3, 3], [1, 4], [4, 1], [2, 4], [4, 2]]   # 13 custom steps: 16 with the defaults

# name -> dict(kind 'C' | 'XY', N, M, cost, kw, tile, seed, and for 'XY': K, lead, dtype, one_d)
CASES = {}


def _add(name, kind, N, M, *, cost="rand", tile=0, seed=None, K=12, lead=(), dtype="float64", one_d=False, **kw):
    CASES[name] = dict(kind=kind, N=int(N), M=int(M), cost=cost, kw=kw, tile=int(tile), seed=7000 + len(CASES) if seed is None else seed, K=int(K), lead=tuple(lead), dtype=dtype, one_d=one_d)


# tile edges: one cell, one row, one column, just below / at / just above the tile, two and three tiles a side (129 x 130: a 3 x 3 grid); random
# costs and integer costs in {0, 1, 2}, whose exact ties let the order of the candidates decide
for _N, _M in ((1, 1), (1, 70), (70, 1), (63, 65), (64, 64), (65, 130), (130, 65), (129, 130)):
    _add(f"c_{_N}x{_M}_rand", "C", _N, _M)
    _add(f"c_{_N}x{_M}_ints", "C", _N, _M, cost="ints")
# forced tiles: many-tile grids at tiny shapes; bit-equal to the default tile's
_add("t8_20x37", "C", 20, 37, cost="ints", tile=8)
_add("t8_37x20", "C", 37, 20, tile=8)
_add("t16_65x70", "C", 65, 70, cost="ints", tile=16)
_add("t32_65x70", "C", 65, 70, tile=32)
# step tables: the defaults carry infinite weights and the integer costs hold zeros (inf * 0 = NaN, the candidate that loses every <)
_add("s121_65x70", "C", 65, 70, cost="ints", step_sizes_sigma=[[1, 1], [1, 2], [2, 1]])
_add("s121w_65x70", "C", 65, 70, cost="ints", step_sizes_sigma=[[1, 1], [1, 2], [2, 1]], weights_add=[0.5, 1.0, 2.0], weights_mul=[1.0, 2.0, 0.5])
_add("s313_66x90", "C", 66, 90, step_sizes_sigma=[[1, 1], [3, 1], [1, 3]])
_add("s313_t8_66x90", "C", 66, 90, cost="ints", tile=8, step_sizes_sigma=[[1, 1], [3, 1], [1, 3]])
_add("wdef_65x70", "C", 65, 70, weights_add=[0.25, 0.5, 0.125], weights_mul=[2.0, 1.5, 3.0])
_add("neg_sub_33x70", "C", 33, 70, cost="neg", subseq=True)
_add("s8_40x47", "C", 40, 47, step_sizes_sigma=[[1, 1], [8, 1], [1, 8]])
_add("s8_t8_40x47", "C", 40, 47, cost="ints", tile=8, step_sizes_sigma=[[1, 1], [8, 1], [1, 8]])
_add("s16_30x33", "C", 30, 33, cost="ints", step_sizes_sigma=STEPS_16)
# subseq: N < M; a given C with more rows than columns (wp flipped, D not transposed); N > M with X / Y is xy_sub_130x70 below
_add("sub_33x70", "C", 33, 70, subseq=True)
_add("sub_70x33", "C", 70, 33, subseq=True)
_add("sub_ints_65x130", "C", 65, 130, cost="ints", subseq=True)
# the Sakoe-Chiba band, applied as a predicate
for _N, _M in ((40, 50), (50, 40)):
    _add(f"gc_{_N}x{_M}", "C", _N, _M, global_constraints=True, band_rad=0.2)
    _add(f"gc_sub_{_N}x{_M}", "C", _N, _M, global_constraints=True, band_rad=0.2, subseq=True)
_add("gc_t8_40x50", "C", 40, 50, cost="ints", tile=8, global_constraints=True, band_rad=0.2)
_add("gc0_sub_20x37", "C", 20, 37, global_constraints=True, band_rad=0.0, subseq=True)   # (radius 0 masks (0, 0) and leaves a band beside the diagonal: a path only under subseq)
# other types of a given C (converted exactly)
_add("c_f32_20x37", "C", 20, 37, dtype="float32")
_add("c_i32_20x37", "C", 20, 37, cost="ints", dtype="int32")
_add("c_i64_20x37", "C", 20, 37, cost="ints", dtype="int64")
_add("c_u8_20x37", "C", 20, 37, cost="ints", dtype="uint8")
_add("c_i16_20x37", "C", 20, 37, cost="ints", dtype="int16")
# X / Y: every metric at 12 x 130 against 12 x 70; subseq with the longer X (D transposed, wp flipped); 1-D; a lead shape; float32
for _metric in METRICS:
    _add(f"xy_{_metric}", "XY", 130, 70, metric=_metric)
_add("xy_sub_130x70", "XY", 130, 70, subseq=True)
_add("xy_sub_70x130", "XY", 70, 130, subseq=True, metric="cosine")
_add("xy_1d", "XY", 40, 30, one_d=True, K=1)
_add("xy_lead", "XY", 65, 40, lead=(2,), metric="cityblock")
_add("xy_f32", "XY", 65, 40, dtype="float32")
_add("xy_s121", "XY", 65, 70, metric="sqeuclidean", step_sizes_sigma=[[1, 1], [1, 2], [2, 1]], weights_mul=[1.0, 2.0, 2.0])

GIVEN = [n for n, c in CASES.items() if c["kind"] == "C"]
FEATURES = [n for n, c in CASES.items() if c["kind"] == "XY"]

# name -> (the case whose model steps are walked, kwargs of dtw_backtracking)
BACKTRACKS = {
    "bt_plain": ("c_63x65_ints", {}),
    "bt_plain_tiles": ("c_129x130_rand", {}),
    "bt_sub": ("sub_33x70", dict(subseq=True)),
    "bt_sub_start": ("sub_33x70", dict(subseq=True, start=17)),
    "bt_sub_start0": ("sub_ints_65x130", dict(subseq=True, start=0)),
    "bt_s313": ("s313_66x90", dict(step_sizes_sigma=[[1, 1], [3, 1], [1, 3]])),
}


def inputs(name):
    """The arguments of a case: dict(C=..., kw) or dict(X=..., Y=..., kw)."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    N, M = c["N"], c["M"]
    if c["kind"] == "C":
        if c["cost"] == "rand":
            C = rng.random((N, M))
        elif c["cost"] == "ints":
            C = rng.integers(0, 3, size=(N, M)).astype(np.float64)
        elif c["cost"] == "neg":
            C = rng.random((N, M)) - 0.5
        else:
            raise KeyError(c["cost"])
        return dict(C=C.astype(c["dtype"]), kw=dict(c["kw"]))
    if c["one_d"]:
        X, Y = rng.random(N), rng.random(M)
    else:
        X, Y = rng.random(c["lead"] + (c["K"], N)), rng.random(c["lead"] + (c["K"], M))
    return dict(X=X.astype(c["dtype"]), Y=Y.astype(c["dtype"]), kw=dict(c["kw"]))


def step_table(kw):
    """The reference's concatenated step table and weights of a call's keyword arguments (:307-337)."""
    sigma, w_add, w_mul = kw.get("step_sizes_sigma"), kw.get("weights_add"), kw.get("weights_mul")
    if sigma is None:
        return DEFAULT_STEPS.copy(), np.zeros(3) if w_add is None else np.asarray(w_add, float), np.ones(3) if w_mul is None else np.asarray(w_mul, float)
    sigma = np.asarray(sigma)
    w_add = np.zeros(len(sigma)) if w_add is None else np.asarray(w_add, float)
    w_mul = np.ones(len(sigma)) if w_mul is None else np.asarray(w_mul, float)
    return np.concatenate((DEFAULT_STEPS, sigma)), np.concatenate((np.full(3, np.inf), w_add)), np.concatenate((np.full(3, np.inf), w_mul))


def band_mask(N, M, band_rad):
    """util.fill_off_diagonal's cells (util/utils.py:2050-2067) as a predicate on m - n."""
    radius = int(np.round(band_rad * min(N, M)))
    offset = abs(N - M)
    d = np.arange(M)[None, :] - np.arange(N)[:, None]
    if N < M:
        return (d >= radius + offset) | (d <= -radius)
    return (d >= radius) | (d <= -radius - offset)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
def model(C, kw):
    """``D`` (float64) and ``steps`` (int32) of a cost matrix under a call's keyword arguments, one anti-diagonal at a time."""
    steps, w_add, w_mul = step_table(kw)
    C = np.atleast_2d(np.asarray(C)).astype(np.float64)
    N, M = C.shape
    if kw.get("global_constraints"):
        C = np.where(band_mask(N, M, kw.get("band_rad", 0.25)), np.inf, C)
    max0, max1 = int(steps[:, 0].max()), int(steps[:, 1].max())
    D = np.full((N + max0, M + max1), np.inf)
    D[max0, max1] = C[0, 0]
    if kw.get("subseq"):
        D[max0, max1:] = C[0, :]
    S = np.zeros((N, M), dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for d in range(N + M - 1):
            n = np.arange(max(0, d - M + 1), min(N - 1, d) + 1)
            m = d - n
            cv = C[n, m]
            best = D[n + max0, m + max1].copy()
            bs = np.zeros(len(n), dtype=np.int32)
            for i, (s0, s1) in enumerate(steps):
                cur = w_mul[i] * cv
                cur = cur + w_add[i]
                cost = D[n + max0 - s0, m + max1 - s1] + cur
                better = cost < best
                best = np.where(better, cost, best)
                bs = np.where(better, i, bs)
            D[n + max0, m + max1] = best
            S[n, m] = bs
    return D[max0:, max1:].copy(), S


def model_backtrack(S, steps, subseq=False, start=None):
    """``__dtw_backtracking`` (:575-640) in Python integers."""
    n, m = S.shape[0] - 1, S.shape[1] - 1 if start is None else int(start)
    wp = [(n, m)]
    while (subseq and n > 0) or (not subseq and (n, m) != (0, 0)):
        s = int(S[n, m])
        n, m = n - int(steps[s][0]), m - int(steps[s][1])
        if min(n, m) < 0:
            break
        wp.append((n, m))
    return np.asarray(wp, dtype=np.int64).reshape(-1, 2)


def model_dtw(C, kw):
    """What ``dtw(C=C, return_steps=True, **kw)`` returns, by the model: (D, wp, steps)."""
    D, S = model(C, kw)
    steps = step_table(kw)[0]
    if kw.get("subseq"):
        wp = model_backtrack(S, steps, True, int(np.argmin(D[-1])))
        if D.shape[0] > D.shape[1]:
            wp = np.fliplr(wp)
    else:
        wp = model_backtrack(S, steps)
    return D, wp, S


def np_cost(X, Y, metric):
    """The cost matrix of a feature pair in NumPy float64, the features in ``X.reshape(-1, N)``'s order (within eps_C of scipy's cdist)."""
    X = np.atleast_2d(X).astype(np.float64)
    Y = np.atleast_2d(Y).astype(np.float64)
    X, Y = X.reshape(-1, X.shape[-1]), Y.reshape(-1, Y.shape[-1])
    diff = X[:, :, None] - Y[:, None, :]
    if metric == "euclidean":
        return np.sqrt((diff * diff).sum(axis=0))
    if metric == "sqeuclidean":
        return (diff * diff).sum(axis=0)
    if metric == "cityblock":
        return np.abs(diff).sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        cs = (X.T @ Y) / (np.sqrt((X * X).sum(axis=0))[:, None] * np.sqrt((Y * Y).sum(axis=0))[None, :])
    return 1.0 - np.clip(cs, -1.0, 1.0)


def eps_c(metric, K, R):
    """The module docstring's bound on the distance between two float64 evaluations of a metric: K features of magnitude up to R."""
    u = 2.0 ** -53
    if metric == "sqeuclidean":
        return 2 * (K + 2) * u * K * (2 * R) ** 2
    if metric == "euclidean":
        return 2 * (K + 3) * u * np.sqrt(K) * 2 * R
    if metric == "cityblock":
        return 2 * (K + 1) * u * K * 2 * R
    if metric == "cosine":
        return 2 * (2 * K + 8) * u
    raise KeyError(metric)


def delta(name, D):
    """How far a cell of D can move under the device's own cost matrix (the module docstring)."""
    c, a = CASES[name], inputs(name)
    K = int(np.prod(c["lead"], dtype=int)) * c["K"]
    R = float(max(np.abs(a["X"]).max(), np.abs(a["Y"]).max()))
    w_mul = step_table(a["kw"])[2]
    w_max = float(np.max(np.abs(w_mul[np.isfinite(w_mul)])))
    d_max = float(np.max(np.abs(D[np.isfinite(D)]), initial=1.0))
    return (c["N"] + c["M"] - 1) * (w_max * eps_c(a["kw"].get("metric", "euclidean"), K, R) + 3 * np.spacing(d_max))


def margin(C, kw, D, wp_unflipped):
    """The smallest gap between the chosen and the next candidate over the cells of a path (its last cell takes no step), and under subseq the gap
    of the final argmin.  C: the cost matrix the path was found on; wp_unflipped: pairs (n, m) of D's own axes."""
    steps, w_add, w_mul = step_table(kw)
    N, M = D.shape
    if kw.get("global_constraints"):
        C = np.where(band_mask(N, M, kw.get("band_rad", 0.25)), np.inf, C)
    gap = np.inf
    with np.errstate(invalid="ignore"):
        for n, m in wp_unflipped[:-1]:
            costs = []
            for i, (s0, s1) in enumerate(steps):
                cur = w_mul[i] * C[n, m]
                cur = cur + w_add[i]
                pn, pm = n - s0, m - s1
                costs.append((D[pn, pm] if pn >= 0 and pm >= 0 else np.inf) + cur)
            if kw.get("subseq") and n == 0:
                costs.append(C[0, m])
            costs = np.sort(np.asarray(costs)[~np.isnan(costs)])
            assert costs[0] == D[n, m]
            if costs.size > 1:
                gap = min(gap, float(costs[1] - costs[0]))
        if kw.get("subseq") and M > 1:
            last = np.sort(D[-1])
            gap = min(gap, float(last[1] - last[0]))
    return gap


# ---- refused calls ------------------------------------------------------------------------------------------------------------------------------
def refusals():
    """name -> (function name, args, kw, needs_device): calls the reference refuses with a ParameterError whose text the golden holds."""
    rng = np.random.default_rng(78)
    C = rng.random((6, 9))
    X, Y = rng.random((3, 6)), rng.random((3, 9))
    nan = C.copy()
    nan[4, 7] = np.nan
    S = np.zeros((6, 9), dtype=np.int32)
    return {
        "c_and_x": ("dtw", (X,), dict(C=C), False),
        "c_and_xy": ("dtw", (X, Y), dict(C=C), False),
        "neither": ("dtw", (), {}, False),
        "x_alone": ("dtw", (X,), {}, False),
        "negative_steps": ("dtw", (), dict(C=C, step_sizes_sigma=[[1, 1], [-1, 2]]), False),
        "weights_add_length": ("dtw", (), dict(C=C, step_sizes_sigma=[[1, 1], [1, 2]], weights_add=[0.0]), False),
        "weights_mul_length": ("dtw", (), dict(C=C, step_sizes_sigma=[[1, 1], [1, 2]], weights_mul=[1.0, 1.0, 1.0]), False),
        "weights_default_steps_length": ("dtw", (), dict(C=C, weights_add=[0.0, 0.0]), False),
        "feature_counts": ("dtw", (X, rng.random((4, 9))), {}, False),
        "nan_in_c": ("dtw", (), dict(C=nan), True),
        "nan_in_c_subseq_band": ("dtw", (), dict(C=nan, subseq=True, global_constraints=True), True),
        "band_zero": ("dtw", (), dict(C=C, global_constraints=True, band_rad=0.0), True),
        "no_path_diagonal_steps": ("dtw", (), dict(C=C, step_sizes_sigma=[[2, 2]]), True),
        "start_without_subseq": ("dtw_backtracking", (S,), dict(start=3), False),
    }


def limits():
    """name -> (function name, args, kw, a word of the message): the documented differences, refused before any device work."""
    rng = np.random.default_rng(79)
    C = rng.random((6, 9))
    X, Y = rng.random((3, 6)), rng.random((3, 9))
    return {
        "metric": ("dtw", (X, Y), dict(metric="chebyshev"), "metric"),
        "metric_callable": ("dtw", (X, Y), dict(metric=lambda u, v: 0.0), "metric"),
        "zero_step": ("dtw", (), dict(C=C, step_sizes_sigma=[[0, 0]]), "(0, 0)"),
        "component_9": ("dtw", (), dict(C=C, step_sizes_sigma=[[1, 1], [9, 1]]), "component of 9"),
        "steps_17": ("dtw", (), dict(C=C, step_sizes_sigma=STEPS_16 + [[4, 4]]), "17 steps"),
        "bt_zero_step": ("dtw_backtracking", (np.zeros((6, 9), dtype=np.int32),), dict(step_sizes_sigma=[[0, 0]]), "(0, 0)"),
        "bt_start_outside": ("dtw_backtracking", (np.zeros((6, 9), dtype=np.int32),), dict(subseq=True, start=9), "start=9"),
    }


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


_golden = None


def load():
    """(arrays, meta) of tests/golden/dtw.npz."""
    global _golden
    if _golden is None:
        z = np.load(GOLDEN)
        _golden = ({k: z[k] for k in z.files if k != "meta"}, json.loads(str(z["meta"])))
    return _golden


# ---- running and judging a case (host simulator and device alike) --------------------------------------------------------------------------------
def run_case(name, seq, wrap=lambda a: a, tile=None, **more):
    """A case through the package (seq: librosa_amd.sequence; wrap: what turns the signal-sized arguments into the caller's kind of array) with
    return_steps: (D, wp, steps) as returned.  tile: the case's own unless given."""
    c, a = CASES[name], inputs(name)
    old = seq.DTW_TILE
    seq.DTW_TILE = c["tile"] if tile is None else tile
    try:
        if c["kind"] == "C":
            before = a["C"].copy()
            out = seq.dtw(C=wrap(a["C"]), return_steps=True, **a["kw"], **more)
            assert np.array_equal(before, a["C"]), "the input was written"
        else:
            bx, by = a["X"].copy(), a["Y"].copy()
            out = seq.dtw(wrap(a["X"]), wrap(a["Y"]), return_steps=True, **a["kw"], **more)
            assert np.array_equal(bx, a["X"]) and np.array_equal(by, a["Y"]), "the input was written"
    finally:
        seq.DTW_TILE = old
    return out


def _first_difference(name, D, S):
    a = inputs(name)
    mD, mS = model(a["C"], a["kw"])
    bad = np.argwhere(~((D == mD) | (np.isnan(D) & np.isnan(mD))) | (S != mS))
    if not len(bad):
        return "equal to the model"
    n, m = bad[np.argmin(bad.sum(axis=1))]
    return f"first cell off the model (by anti-diagonal): ({n}, {m}): D {D[n, m]!r} against {mD[n, m]!r}, step {S[n, m]} against {mS[n, m]}; {len(bad)} cells differ"


def d_error(a, b):
    """The largest distance between two rows of D; cells infinite in both count as equal, a cell infinite in one alone as NaN (which fails)."""
    with np.errstate(invalid="ignore"):
        return float(np.max(np.where(a == b, 0.0, np.abs(a - b))))


def check_case(name, D, wp, steps, report=None):
    """The two rules of dtw_cases against the golden; returns the worst error of D on the stored row and column (0 for the bit-equal rule)."""
    arrays, meta = load()
    c = CASES[name]
    g_wp, g_row, g_col = arrays[f"{name}/wp"], arrays[f"{name}/row"], arrays[f"{name}/col"]
    assert D.dtype == np.float64 and wp.dtype == np.int64 and steps.dtype == np.int32
    assert list(D.shape) == meta["cases"][name]["shape"] and steps.shape == D.shape and wp.ndim == 2 and wp.shape[1] == 2
    if c["kind"] == "C":
        ok = sha(D) == meta["cases"][name]["sha_D"] and sha(steps) == meta["cases"][name]["sha_steps"]
        assert ok, f"{name}: D or steps is not bit-equal to the reference's; {_first_difference(name, D, steps)}"
        assert np.array_equal(D[-1], g_row) and np.array_equal(D[:, -1], g_col)
        assert np.array_equal(wp, g_wp), f"{name}: wp"
        return 0.0
    d = meta["cases"][name]["delta"]
    err = max(d_error(D[-1], g_row), d_error(D[:, -1], g_col), key=lambda e: (e != e, e))
    if report is not None:
        report(f"{name}: worst D error {err:.3g} (bound {d:.3g}, margin {meta['cases'][name]['margin']:.3g})")
    assert np.array_equal(wp, g_wp), f"{name}: wp"
    assert err <= d, f"{name}: D off by {err:.3g}, bound {d:.3g}"
    return err
