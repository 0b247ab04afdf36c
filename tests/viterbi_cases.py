"""Cases, inputs and the NumPy model of ``sequence.viterbi`` and its variants, shared by ``scripts/make_viterbi_golden.py``,
``tests/test_viterbi_host.py`` and ``tests/test_viterbi_gpu.py``.

TEST INFRASTRUCTURE ONLY.  Inputs come from seeds.  ``tests/golden/viterbi.npz`` holds the unmodified reference's states and ``logp`` of every
case (``_viterbi`` itself for the log-domain cases), the ``transition_*`` tables, the messages of the refused calls and, per case, the margin.

The model (``model``) is the reference's recursion with the loop over targets vectorised: ``np.argmax(value[:, None] + log_trans, axis=0)`` per
step.  Every operation is one float64 addition or a comparison and ``np.argmax`` takes the first maximum, so the model gives the reference's
bits; the host test asserts that for every case.

Two rules.
  * Log-domain path (``sequence._viterbi_log``, the log tables computed here with NumPy exactly as the reference computes them): states and
    ``logp`` are bit-equal to the golden.
  * Public path: the device takes the logarithm of ``prob`` itself, within 2 ulp of NumPy's.  A log of a value in [tiny, 1] is at most 709 in
    magnitude (88 for float32), each of the T steps adds one observation (2 ulp of 709: ``4 * 2**-52 * 709``) and rounds twice at the size of the
    running value, so no ``value`` moves further than ``delta = T * (4 * 2**-52 * 709 + 2 * ulp(|logp|))`` (``delta32 = T * (2 * 2**-24 * 88 +
    2 * ulp(|logp|))`` for float32 ``prob``).  The MARGIN of a case is the smallest gap between the best and the runner-up candidate over the
    decisions on the decoded path, together with the gap of the final argmax.  Every public-path case is certified: ``margin >= 1e-6`` and
    ``margin >= 4 * delta``; then the states are equal and ``logp`` is within ``delta``.  A case that fails certification gets another seed.
"""
from __future__ import annotations

import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "viterbi.npz")
SMALL_MAX = 32        # states of the small kernel (csrc/lra_viterbi.h: kSmallMax)
MAX_STATES = 8192     # csrc/lra_viterbi.h: kMaxStates
PREP_STEPS = 32       # the prepare kernel's step tile (kPrepSteps)
SMALL_CHAINS = 128    # the most chains a workgroup of the small kernel holds (2 states: kSmallNT / 2)
MARGIN_FLOOR, MARGIN_FACTOR = 1e-6, 4.0

# name -> dict(fn, S, T, lead, thr, dtype, p_init, p_state, trans, seed)
CASES = {}


def _add(name, fn, S, T, *, lead=(), thr=None, dtype="float64", p_init=False, p_state=False, trans="dirichlet", seed=None):
    CASES[name] = dict(fn=fn, S=int(S), T=int(T), lead=None if lead is None else tuple(lead), thr=thr, dtype=dtype, p_init=p_init, p_state=p_state, trans=trans, seed=9000 + len(CASES) if seed is None else seed)


# states: the small-kernel boundary, the lane splits of the workgroup kernel (64 / 128), one target per thread, several per thread
for _S in (1, 2, 3, 31, 32, 33, 63, 64, 65, 257, 1025):
    _T = 3 if _S == 1025 else 6 if _S == 257 else 20
    _add(f"v_s{_S}", "viterbi", _S, _T)
    _add(f"d_s{_S}_thr", "discriminative", _S, _T, thr=0.25 / _S, trans="diag")
# steps: 1, 2 and around the prepare kernel's tile, in both decode kernels
for _T in (1, 2, PREP_STEPS - 1, PREP_STEPS, PREP_STEPS + 1):
    _add(f"v_t{_T}", "viterbi", 5, _T)
    _add(f"d_t{_T}", "discriminative", 40, _T)
_add("v_lead3", "viterbi", 7, 10, lead=(3,))
_add("d_lead23", "discriminative", 40, 9, lead=(2, 3))
_add("v_lead23_thr", "viterbi", 70, 9, lead=(2, 3), thr=0.25 / 70, trans="diag")
_add("v_many", "viterbi", 2, 6, lead=(SMALL_CHAINS + 2,))
# pyin's transition: two blocks (voiced, unvoiced) of a triangular band, thresholded at 1e-4
_add("pyin_242", "viterbi", 242, 40, thr=1e-4, trans="pyin", p_init=True)
_add("pyin_1200", "viterbi", 1200, 5, thr=1e-4, trans="pyin")
_add("v_pinit", "viterbi", 6, 20, p_init=True)
_add("d_pstate", "discriminative", 6, 20, p_init=True, p_state=True)
_add("d_pstate_wg", "discriminative", 40, 12, p_state=True)
_add("b_shared5", "binary", 5, 30, trans="shared")
_add("b_tables70", "binary", 70, 12, lead=(2,), trans="tables", p_init=True, p_state=True)
_add("b_1d", "binary", 1, 10, trans="shared", lead=None)
_add("b_thr", "binary", 5, 20, trans="tables", thr=0.05)
_add("v_f32", "viterbi", 5, 40, dtype="float32")
# log-domain only
_add("log_uniform", "log", 40, 8, trans="uniform")
_add("log_uniform_small", "log", 4, 8, trans="uniform")
_add("log_ties_small", "log", 5, 12, trans="ints", lead=(3,))
_add("log_ties_split", "log", 70, 8, trans="ints")
_add("log_ties_wg", "log", 300, 4, trans="ints")
_add("log_ties_thr", "log", 70, 8, trans="ints", thr=-2.0)
_add("log_zeros", "log", 40, 10, trans="zeros")
_add("log_neginf", "log", 40, 6, trans="neginf")
_add("log_neginf_small", "log", 4, 6, trans="neginf")
_add("log_max_states", "log", MAX_STATES, 3, trans="band", thr=-20.0)

PUBLIC = [n for n, c in CASES.items() if c["fn"] != "log"]
LOG = [n for n, c in CASES.items() if c["fn"] == "log"]


def _triangle_band(n, width):
    """A row-normalised triangular band of `width` states around the diagonal (the shape of transition_local(n, width, 'triangle'))."""
    i = np.arange(n)
    d = np.abs(i[:, None] - i[None, :])
    t = np.maximum(0.0, 1.0 - d / ((width + 1) / 2.0))
    return t / t.sum(axis=1, keepdims=True)


def _loop2(p):
    return np.array([[p, 1 - p], [1 - p, p]])


def inputs(name):
    """The arguments of a case: dict(prob, transition, kw) for the public functions; dict(log_prob, log_trans, log_p_init, thr) for 'log'."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    S, T, fn = c["S"], c["T"], c["fn"]
    lead = () if c["lead"] is None else c["lead"]
    if fn == "log":
        return _log_inputs(c, rng)
    kw = {}
    if c["thr"] is not None:
        kw["transition_min_prob"] = c["thr"]
    if fn == "binary":
        prob = rng.uniform(0.02, 0.98, size=lead + (S, T))
        if c["lead"] is None:
            prob = prob[0]
        one = lambda: np.array([rng.dirichlet([6.0, 2.0]), rng.dirichlet([2.0, 6.0])])
        transition = one() if c["trans"] == "shared" else np.stack([one() for _ in range(S)])
        if c["p_init"]:
            kw["p_init"] = rng.uniform(0.1, 0.9, size=S)
        if c["p_state"]:
            kw["p_state"] = rng.uniform(0.1, 0.9, size=S)
        return dict(prob=prob, transition=transition, kw=kw)
    prob = np.swapaxes(rng.dirichlet(np.ones(S), size=lead + (T,)), -1, -2).astype(c["dtype"])
    if c["dtype"] != "float64":   # (a float32 column of a discriminative case would still sum to 1 within allclose)
        prob = np.ascontiguousarray(prob)
    if c["trans"] == "dirichlet":
        transition = rng.dirichlet(np.ones(S), size=S)
    elif c["trans"] == "diag":
        transition = 0.5 * np.eye(S) + 0.5 * rng.dirichlet(np.ones(S), size=S)
    elif c["trans"] == "pyin":
        half = S // 2
        transition = np.kron(_loop2(0.99), _triangle_band(half, half // 5 + 1))
    else:
        raise KeyError(c["trans"])
    if c["p_init"]:
        kw["p_init"] = rng.dirichlet(np.ones(S))
    if c["p_state"]:
        kw["p_state"] = rng.dirichlet(4.0 * np.ones(S))
    return dict(prob=np.ascontiguousarray(prob), transition=transition, kw=kw)


def band_lists(S):
    """log_max_states: every target's predecessors j - 2 .. j + 2 (inside the range), ascending, as (k [e][j], log_trans [e][j], lengths)."""
    j = np.arange(S)
    rows_k, rows_v = [], []
    for d in (-2, -1, 0, 1, 2):
        rows_k.append(j + d)
        rows_v.append(-1.0 - 0.25 * ((j * 7 + d * 3) % 5))
    k, v = np.stack(rows_k), np.stack(rows_v)
    ok = (k >= 0) & (k < S)
    order = np.argsort(~ok, axis=0, kind="stable")   # the valid ones first, still ascending
    k, v, ok = np.take_along_axis(k, order, 0), np.take_along_axis(v, order, 0), np.take_along_axis(ok, order, 0)
    return np.where(ok, k, 0), np.where(ok, v, -np.inf), ok.sum(axis=0)


def band_dense(S):
    k, v, n = band_lists(S)
    dense = np.full((S, S), -np.inf)
    for e in range(k.shape[0]):
        j = np.flatnonzero(e < n)
        dense[k[e, j], j] = v[e, j]
    return dense


def _log_inputs(c, rng):
    S, T, lead, kind = c["S"], c["T"], c["lead"], c["trans"]
    thr = -np.inf if c["thr"] is None else float(c["thr"])
    tiny = np.finfo(np.float64).tiny
    if kind == "uniform":
        lp, lt, pi = np.zeros(lead + (S, T)), np.full((S, S), np.log(1.0 / S)), np.full(S, np.log(1.0 / S))
    elif kind == "ints":   # small integers: every sum is exact, and equal costs at unequal indices are everywhere
        lp = rng.integers(-3, 1, size=lead + (S, T)).astype(np.float64)
        lt = rng.integers(-3, 1, size=(S, S)).astype(np.float64)
        lt[np.arange(S), np.arange(S)] = 0.0   # (the thresholded variant keeps every target's list non-empty)
        pi = rng.integers(-2, 1, size=S).astype(np.float64)
    elif kind == "zeros":   # probability zeros through the reference's own logarithm
        prob = rng.dirichlet(np.ones(S), size=lead + (T,)).swapaxes(-1, -2) * (rng.random(lead + (S, T)) < 0.6)
        trans = rng.dirichlet(np.ones(S), size=S) * (rng.random((S, S)) < 0.5)
        lp, lt, pi = np.log(prob + tiny), np.log(trans + tiny), np.log(np.full(S, 1.0 / S) + tiny)
    elif kind == "neginf":  # target 0 has no finite candidate and the last step leaves every value at -inf: argmax 0, pointers 0 all the way
        lp = np.log(rng.dirichlet(np.ones(S), size=lead + (T,)).swapaxes(-1, -2))
        lp[..., 1:, T - 1] = -np.inf
        lt = np.log(rng.dirichlet(np.ones(S), size=S))
        lt[:, 0] = -np.inf
        pi = np.log(np.full(S, 1.0 / S))
    elif kind == "band":
        lp = np.log(rng.dirichlet(np.ones(64), size=(T, S // 64)).reshape(T, S).T / 128.0)
        lt = None   # (dense S x S: built where it is needed, band_dense(S))
        pi = np.log(rng.dirichlet(np.ones(64), size=S // 64).reshape(S) / 128.0)
    else:
        raise KeyError(kind)
    return dict(log_prob=np.ascontiguousarray(lp), log_trans=lt, log_p_init=pi, thr=thr)


# ---- the reference's host tables ----------------------------------------------------------------------------------------------------------------
def log_tables(name):
    """What the reference hands to ``_viterbi`` for a public-path case, computed with NumPy as it computes them: log_prob (chains, S, T) float64
    (exactly widened), log_trans (tables, S, S), log_p_init (tables, S), the threshold; for 'binary' the chains are (item, label) pairs of 2 states."""
    c, a = CASES[name], inputs(name)
    prob, transition, kw = a["prob"], a["transition"], a["kw"]
    fn, S = c["fn"], c["S"]
    tmp = kw.get("transition_min_prob")
    if fn == "binary":
        prob = np.atleast_2d(prob)
        eps = np.finfo(np.float64).tiny
        if transition.shape == (2, 2):
            transition = np.tile(transition, (S, 1, 1))
        pair = lambda p: np.stack([1 - p, p], axis=-1)
        p_state = kw.get("p_state", np.full(S, 0.5))
        p_init = kw.get("p_init", np.full(S, 0.5))
        both = np.stack([1 - prob, prob], axis=-2).astype(np.float64)       # (..., label, 2, T)
        lp = np.log(both + eps) - np.log(pair(p_state) + eps)[..., None]
        thr = np.log(tmp + eps) if tmp else -np.inf
        return lp.reshape((-1, 2, c["T"])), np.log(transition + eps), np.log(pair(p_init) + eps), thr
    eps = np.finfo(prob.dtype).tiny
    p_init = kw.get("p_init", np.full(S, 1.0 / S))
    lp = np.log(prob + eps)
    if fn == "discriminative":
        lp = lp - np.log(kw.get("p_state", np.full(S, 1.0 / S)) + eps)[:, None]
    thr = np.log(tmp + eps) if tmp else -np.inf
    return lp.astype(np.float64).reshape((-1, S, c["T"])), np.log(transition + eps)[None], np.log(p_init + eps)[None], thr


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
def _gap(costs):
    """best minus runner-up of a row of candidate costs (inf for a single candidate; 0 on a tie; nan-free inputs)."""
    if costs.size < 2:
        return np.inf
    top = np.partition(costs, costs.size - 2)[-2:]
    g = top[1] - top[0]
    return 0.0 if np.isnan(g) else float(g)


def model(log_prob, log_trans, log_p_init, thr=-np.inf):
    """``_viterbi`` of one sequence, log_prob (S, T): states (T,) uint16, logp (1,) float64, and the margin of the decoded path."""
    S, T = log_prob.shape
    lt = log_trans if not np.isfinite(thr) else np.where(log_trans >= thr, log_trans, -np.inf)   # (a cost of -inf never replaces the best: as if not listed)
    value = np.empty((T, S))
    ptr = np.zeros((T, S), dtype=np.uint16)
    value[0] = log_prob[:, 0] + log_p_init
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            cost = value[t - 1][:, None] + lt
            ptr[t] = np.argmax(cost, axis=0)
            value[t] = log_prob[:, t] + cost[ptr[t], np.arange(S)]
        states = np.zeros(T, dtype=np.uint16)
        states[-1] = np.argmax(value[-1])
        margin = _gap(value[-1])
        for t in range(T - 2, -1, -1):
            states[t] = ptr[t + 1, states[t + 1]]
            col = value[t] + lt[:, states[t + 1]]
            if np.isfinite(thr):
                col = col[log_trans[:, states[t + 1]] >= thr]
            margin = min(margin, _gap(col))
    return states, value[-1:, states[-1]].copy(), margin


def model_lists(log_prob, pred_k, pred_lt, pred_n, log_p_init):
    """The same recursion over predecessor lists (k [e][j], log_trans [e][j] with -inf beyond a list's length): the sparse model of log_max_states."""
    S, T = log_prob.shape
    value = log_prob[:, 0] + log_p_init
    ptrs = []
    for t in range(1, T):
        cost = value[pred_k] + pred_lt
        e = np.argmax(cost, axis=0)
        best = cost[e, np.arange(S)]
        ptrs.append(np.where(best > -np.inf, pred_k[e, np.arange(S)], 0))
        value = log_prob[:, t] + best
    states = np.zeros(T, dtype=np.uint16)
    states[-1] = np.argmax(value)
    for t in range(T - 2, -1, -1):
        states[t] = ptrs[t][states[t + 1]]
    return states, np.array([value[states[-1]]])


def model_case(name):
    """The model over every chain of a case: states (chains, T), logp (chains,), margin (the smallest over the chains)."""
    c = CASES[name]
    if c["fn"] == "log":
        a = inputs(name)
        lp = a["log_prob"].reshape((-1, c["S"], c["T"]))
        if a["log_trans"] is None:
            res = [model_lists(x, *band_lists(c["S"]), a["log_p_init"]) + (np.inf,) for x in lp]
        else:
            res = [model(x, a["log_trans"], a["log_p_init"], a["thr"]) for x in lp]
    else:
        lp, lt, pi, thr = log_tables(name)
        res = [model(x, lt[i % len(lt)], pi[i % len(pi)], thr) for i, x in enumerate(lp)]
    return np.stack([r[0] for r in res]), np.array([r[1][0] for r in res]), min(r[2] for r in res)


def delta(name, logp):
    """How far the device's own logarithms can move a value of the case (the module docstring)."""
    c = CASES[name]
    worst = float(np.max(np.abs(logp[np.isfinite(logp)]), initial=1.0))
    if c["dtype"] == "float32":
        return c["T"] * (2 * 2.0 ** -24 * 88 + 2 * np.spacing(worst))
    return c["T"] * (4 * 2.0 ** -52 * 709 + 2 * np.spacing(worst))


def out_shapes(name):
    """The shapes the reference returns: (states, logp)."""
    c = CASES[name]
    lead = () if c["lead"] is None else c["lead"]
    if c["fn"] == "binary":
        return lead + (c["S"], c["T"]), lead + (c["S"],)
    if c["fn"] == "viterbi":
        return lead + (c["T"],), lead if lead else (1,)
    if c["fn"] == "discriminative":
        return lead + (c["T"],), lead
    return lead + (c["T"],), lead + (1,)


# ---- the transition builders --------------------------------------------------------------------------------------------------------------------
BUILDERS = {
    "uniform_1": ("transition_uniform", (1,), {}),
    "uniform_7": ("transition_uniform", (7,), {}),
    "loop_scalar": ("transition_loop", (5, 0.9), {}),
    "loop_vector": ("transition_loop", (3, [0.8, 0.5, 0.25]), {}),
    "cycle_scalar": ("transition_cycle", (4, 0.9), {}),
    "cycle_vector": ("transition_cycle", (3, [0.8, 0.5, 0.25]), {}),
    "local_triangle": ("transition_local", (5, 3), {}),
    "local_wrap": ("transition_local", (5, 3), {"wrap": True}),
    "local_ones_widths": ("transition_local", (5, [1, 2, 3, 3, 1]), {"window": "ones"}),
    "local_hann": ("transition_local", (12, 5), {"window": "hann"}),
    "local_pyin": ("transition_local", (60, 13), {"window": "triangle"}),
}
BUILDER_ERRORS = {
    "uniform_zero": ("transition_uniform", (0,), {}),
    "uniform_float": ("transition_uniform", (2.5,), {}),
    "loop_one": ("transition_loop", (1, 0.5), {}),
    "loop_length": ("transition_loop", (3, [0.5, 0.5]), {}),
    "loop_range": ("transition_loop", (3, 1.5), {}),
    "cycle_one": ("transition_cycle", (1, 0.5), {}),
    "cycle_length": ("transition_cycle", (3, [0.5, 0.5]), {}),
    "cycle_range": ("transition_cycle", (3, -0.5), {}),
    "local_one": ("transition_local", (1, 3), {}),
    "local_length": ("transition_local", (4, [1, 2]), {}),
    "local_width": ("transition_local", (4, 0), {}),
}


# ---- refused calls ------------------------------------------------------------------------------------------------------------------------------
def refusals():
    """name -> (function name, prob, transition, kw, needs_device): calls the reference refuses; the ones marked need the device's range flags."""
    rng = np.random.default_rng(77)
    S, T = 4, 6
    prob = np.swapaxes(rng.dirichlet(np.ones(S), size=T), -1, -2)
    trans = rng.dirichlet(np.ones(S), size=S)
    bprob = rng.uniform(0.1, 0.9, size=(5, T))
    btrans = np.array([[0.9, 0.1], [0.3, 0.7]])
    bad = lambda a, at, v: (lambda b: (b.__setitem__(at, v), b)[1])(a.copy())
    r = {}
    for fn in ("viterbi", "viterbi_discriminative"):
        r[f"{fn}_shape"] = (fn, prob, trans[:3, :3], {}, False)
        r[f"{fn}_negative"] = (fn, prob, bad(trans, (1, 2), -0.1), {}, False)
        r[f"{fn}_rowsum"] = (fn, prob, trans * 0.9, {}, False)
        r[f"{fn}_pinit_negative"] = (fn, prob, trans, dict(p_init=np.array([1.2, -0.2, 0.0, 0.0])), False)
        r[f"{fn}_pinit_sum"] = (fn, prob, trans, dict(p_init=np.full(S, 0.3)), False)
        r[f"{fn}_pinit_shape"] = (fn, prob, trans, dict(p_init=np.full((1, S), 0.25)), False)
        r[f"{fn}_min_prob"] = (fn, prob, trans, dict(transition_min_prob=-0.1), False)
        r[f"{fn}_empty"] = (fn, prob, np.full((S, S), 0.25), dict(transition_min_prob=0.9), False)
        r[f"{fn}_prob_negative"] = (fn, bad(prob, (2, 3), -0.1), trans, {}, True)
    r["viterbi_prob_above"] = ("viterbi", bad(prob, (0, 5), 1.5), trans, {}, True)
    r["viterbi_empty_wg"] = ("viterbi", np.full((40, 3), 1.0 / 40), np.eye(40)[:, ::-1] * 0.5 + 0.5 / 40, dict(transition_min_prob=0.9), False)
    r["viterbi_discriminative_colsum"] = ("viterbi_discriminative", prob * 0.9, trans, {}, True)
    r["viterbi_discriminative_pstate_shape"] = ("viterbi_discriminative", prob, trans, dict(p_state=np.full(S + 1, 0.2)), False)
    r["viterbi_discriminative_pstate_sum"] = ("viterbi_discriminative", prob, trans, dict(p_state=np.full(S, 0.3)), False)
    r["viterbi_binary_shape"] = ("viterbi_binary", bprob, np.tile(btrans, (3, 1, 1)), {}, False)
    r["viterbi_binary_rowsum"] = ("viterbi_binary", bprob, btrans * 1.1, {}, False)
    r["viterbi_binary_pstate"] = ("viterbi_binary", bprob, btrans, dict(p_state=np.full(5, 1.5)), False)
    r["viterbi_binary_pinit"] = ("viterbi_binary", bprob, btrans, dict(p_init=np.full(5, -0.1)), False)
    r["viterbi_binary_min_prob"] = ("viterbi_binary", bprob, btrans, dict(transition_min_prob=-1.0), False)
    r["viterbi_binary_empty"] = ("viterbi_binary", bprob, btrans, dict(transition_min_prob=0.95), False)
    r["viterbi_binary_prob_above"] = ("viterbi_binary", bad(bprob, (4, 1), 1.01), btrans, {}, True)
    r["viterbi_binary_prob_negative"] = ("viterbi_binary", bad(bprob, (0, 0), -0.01), btrans, {}, True)
    return r


_golden = None


def load():
    """(arrays, meta) of tests/golden/viterbi.npz."""
    global _golden
    if _golden is None:
        z = np.load(GOLDEN)
        _golden = ({k: z[k] for k in z.files if k != "meta"}, json.loads(str(z["meta"])))
    return _golden


# ---- running and judging a case (host simulator and device alike) --------------------------------------------------------------------------------
def functions(seq):
    return {"viterbi": seq.viterbi, "discriminative": seq.viterbi_discriminative, "binary": seq.viterbi_binary}


def run_case(name, seq, wrap=lambda a: a):
    """A case through the package (seq: librosa_amd.sequence; wrap: what turns prob into the caller's kind of array): (states, logp) as returned."""
    c, a = CASES[name], inputs(name)
    fns, log_fn = functions(seq), seq._viterbi_log
    if c["fn"] == "log":
        lt = a["log_trans"] if a["log_trans"] is not None else band_dense(c["S"])
        return log_fn(wrap(a["log_prob"]), lt, a["log_p_init"], a["thr"])
    before = a["prob"].copy()
    out = fns[c["fn"]](wrap(a["prob"]), a["transition"], return_logp=True, **a["kw"])
    assert np.array_equal(before, a["prob"]), "the input was written"
    return out


def check_case(name, states, logp, report=None):
    """The two rules of viterbi_cases against the golden; returns the worst logp error."""
    arrays, meta = load()
    g_states, g_logp = arrays[f"{name}/states"], arrays[f"{name}/logp"]
    assert states.dtype == np.uint16 and logp.dtype == np.float64
    assert states.shape == g_states.shape and logp.shape == g_logp.shape
    if CASES[name]["fn"] == "log":
        assert np.array_equal(states, g_states), f"{name}: states"
        assert np.array_equal(logp, g_logp, equal_nan=True) and np.array_equal(np.signbit(logp), np.signbit(g_logp)), f"{name}: logp is not bit-equal"
        return 0.0
    err = float(np.max(np.abs(logp - g_logp), initial=0.0))
    if report is not None:
        report(f"{name}: worst logp error {err:.3g} (bound {meta['cases'][name]['delta']:.3g})")
    assert np.array_equal(states, g_states), f"{name}: states"
    assert err <= meta["cases"][name]["delta"], f"{name}: logp off by {err:.3g}, bound {meta['cases'][name]['delta']:.3g}"
    return err
