"""Sequence decoding: ``librosa.sequence``'s Viterbi decoders and transition builders (``librosa/sequence.py:1174-2146``).

``viterbi``, ``viterbi_discriminative`` and ``viterbi_binary`` have the reference's signatures, checks and messages.  The small float64 tables
(``log_trans``, ``log_p_init``, ``log_marginal``, the threshold and the predecessor lists) are built here with NumPy, bit-equal to the
reference's; the signal-sized ``log_prob`` is computed on the device (``csrc/lra_viterbi.h``: ``viterbi_prep``), which also raises the range
flags on ``prob`` that are read before the decode is launched.  Every sequence of a batch is decoded in one launch: a workgroup per sequence
(``viterbi_wg``), or a group of lanes per chain up to 32 states (``viterbi_small``: all labels of ``viterbi_binary`` at once).

Differences from the reference: ``n_states`` above ``MAX_STATES`` raises ``ParameterError`` (a sequence's two value rows live
in the LDS of one workgroup); ``prob`` must be float32 or float64 (other types are converted as NumPy's promotion with ``tiny(prob)`` would);
a float32 ``p_state`` is widened before it is subtracted.

``dtw`` and ``dtw_backtracking`` (``librosa/sequence.py:185-694``) have the reference's signatures, check order, messages and return shapes.  The
step table and its weights are built here as the reference builds them; the cost matrix (``dtw_cost``, or ``dtw_prepare`` for a given ``C``),
the accumulated cost matrix (``dtw_accumulate``: square tiles, one launch per tile anti-diagonal) and the warping path (``dtw_backtrack``) are
computed on the device (``csrc/lra_dtw.h``).  The checks that need signal-sized data -- NaN in ``C``, ``D[-1, -1]`` infinite, every entry of
``D[-1]`` infinite, a path that does not end at ``(0, 0)`` -- come back as status words and raise the reference's texts.  Given ``C``, the
results are the reference's bit for bit; given ``X`` and ``Y``, the device's own cost matrix is within rounding of scipy's.

Differences from the reference for DTW: ``metric`` is one of ``euclidean``, ``sqeuclidean``, ``cityblock``, ``cosine`` (anything
else raises ``ParameterError``: there is no CPU fallback); the features of ``X`` / ``Y`` are summed in ``X.reshape(-1, N)``'s order; a step
``(0, 0)`` is refused; at most ``DTW_MAX_STEPS`` = 16 steps with the three defaults and no step component above ``DTW_MAX_STEP`` = 8;
``dtw_backtracking`` on a ``steps`` matrix holding an index outside the step table, or with ``start`` outside the columns, raises
``ParameterError`` where the reference raises ``IndexError``.

``rqa`` (``librosa/sequence.py:698-1074``) has the reference's signature, check order, texts and return shapes.  The score matrix and the pointers
(``rqa_score``: blocks of ``RQA_ROWS`` rows, one launch per block, one workgroup per strip of ``RQA_STRIP`` columns that recomputes its left
halo), ``np.argmax(score)`` (``rqa_argmax``) and the walk (``rqa_backtrack``) are computed on the device (``csrc/lra_rqa.h``).  float32 and
float64 ``sim`` are scored in their own type and ``score`` is the reference's bit for bit; ``path`` is uint64.

Differences from the reference for RQA: the walk follows the move that was scored -- the device stores its own pointer codes
(0 diagonal, 1 left knight ``(-1, -2)``, 2 up knight ``(-2, -1)``, -1 and -2 as the reference), where the reference numbers the up knight 1 in
column 1, reads it back as the left knight and steps to column -1 (its path is then cut short, or holds ``2**64 - 1``); wherever the
reference's walk stays inside the matrix the two paths agree.  bool and integer ``sim`` of any width are widened to float64 and ``score`` comes
back as float64, equal to the reference's result on ``sim.astype(float64)`` (the reference truncates the score into the integer type).  Complex or
non-numeric ``sim``, ``sim.ndim != 2`` and an empty ``sim`` raise ``ParameterError`` (the reference: ``IndexError`` for an empty one).
"""
from __future__ import annotations

import numpy as np

from . import _arrays, _native
from .filters import get_window
from .util.exceptions import ParameterError
from .util.utils import is_positive_int, is_torch_tensor, pad_center, tiny

__all__ = ["dtw", "dtw_backtracking", "rqa", "viterbi", "viterbi_discriminative", "viterbi_binary", "transition_uniform", "transition_loop", "transition_cycle", "transition_local"]

MAX_STATES = 8192            # LRA_VITERBI_MAX_STATES
_SMALL_MAX = 32              # LRA_VITERBI_SMALL_MAX: up to here the threshold is a comparison in the kernel, beyond it a list
_LDS_MAX = 160 * 1024        # LRA_VITERBI_LDS_MAX
# bytes of log_prob (8 per state and step) and pointer scratch (2) one launch may hold; longer batches are decoded in chunks of whole sequences
SCRATCH_BUDGET = 4 << 30


def _host(x):
    """A host ndarray of a small argument (a tensor comes down; anything else as np.asarray takes it)."""
    if is_torch_tensor(x):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _check_states(n_states):
    if n_states < 1:
        raise ParameterError(f"n_states={n_states} must be at least 1")
    if n_states > MAX_STATES or _native.load_library().lra_viterbi_lds_bytes(int(n_states), 0) > _LDS_MAX:
        # documented difference: the two live value rows of a sequence are held in the LDS of one workgroup
        raise ParameterError(f"n_states={n_states} is too large for the device decoder: at most {MAX_STATES} states are served")


def _threshold(transition_min_prob, epsilon):
    if transition_min_prob is not None and transition_min_prob > 0:
        return np.log(transition_min_prob + epsilon)
    if transition_min_prob is None or transition_min_prob == 0:
        return -np.inf
    raise ParameterError(f"Invalid transition_min_prob={transition_min_prob}, must be None or non-negative.")


def _predecessors(log_trans, threshold):
    """``np.flatnonzero(log_trans[:, j] >= threshold)`` of every target j, ascending, as the padded target-minor lists the kernel reads:
    (k uint16 [e][j], log_trans float64 [e][j], lengths int32 [j]); raises as ``_viterbi`` does for an empty list."""
    mask = log_trans >= threshold
    counts = mask.sum(axis=0)
    empty = np.flatnonzero(counts == 0)
    if empty.size:
        raise ParameterError(f"Empty transition matrix detected for state {int(empty[0])} in Viterbi. Try reducing your minimum transition probability threshold.")
    jj, kk = np.nonzero(mask.T)   # sorted by target, then by predecessor
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    ee = np.arange(jj.size) - starts[jj]
    n_pred, n_states = int(counts.max()), log_trans.shape[0]
    pred_k = np.zeros((n_pred, n_states), dtype=np.uint16)
    pred_lt = np.full((n_pred, n_states), -np.inf, dtype=np.float64)
    pred_k[ee, jj] = kk
    pred_lt[ee, jj] = log_trans[kk, jj]
    return pred_k, pred_lt, counts.astype(np.int32)


def _as_real(prob):
    """prob as float32 or float64 (what ``prob + tiny(prob)`` promotes to), and the epsilon the reference adds."""
    np_dtype = np.dtype(_arrays.numpy_dtype_of(prob))
    epsilon = tiny(np.empty(0, dtype=np_dtype))
    if np_dtype in (np.dtype(np.float32), np.dtype(np.float64)):
        return prob, np_dtype, epsilon
    if np_dtype.kind not in "biu":
        raise ParameterError(f"prob must be float32, float64 or integer-valued, given dtype={np_dtype}")
    real = np.dtype(np.result_type(np_dtype, np.float32))
    if real not in (np.dtype(np.float32), np.dtype(np.float64)):
        real = np.dtype(np.float32)
    return _arrays.cast(prob, real), real, epsilon


def _search_tables(log_trans, log_p_init, threshold, n_states):
    """The tables as contiguous float64 and, for a thresholded search above ``_SMALL_MAX`` states, the predecessor lists (else None); every
    table's empty-list check, in label order, before any device work."""
    log_trans = np.ascontiguousarray(log_trans, dtype=np.float64)
    log_p_init = np.ascontiguousarray(log_p_init, dtype=np.float64)
    lists = None
    if np.isfinite(threshold):
        for table in log_trans:
            if n_states > _SMALL_MAX:
                lists = _predecessors(table, threshold)
            else:
                empty = np.flatnonzero(~(table >= threshold).any(axis=0))
                if empty.size:
                    raise ParameterError(f"Empty transition matrix detected for state {int(empty[0])} in Viterbi. Try reducing your minimum transition probability threshold.")
    return log_trans, log_p_init, lists


def _upload_tables(sess, log_trans, log_p_init, log_marginal, lists):
    """Device pointers of what ``lra_viterbi_exec`` reads: (log_trans or 0, log_p_init, log_marginal or 0, pred_k, pred_lt, pred_n, n_pred)."""
    host = lambda a, dtype: sess.input_raw(_as_like(sess, np.ascontiguousarray(a, dtype=dtype)), dtype)
    lt_ptr = host(log_trans, np.float64) if lists is None else 0
    pi_ptr = host(log_p_init, np.float64)
    lm_ptr = host(log_marginal, np.float64) if log_marginal is not None else 0
    k_ptr, plt_ptr, n_ptr = (host(lists[0], np.uint16), host(lists[1], np.float64), host(lists[2], np.int32)) if lists is not None else (0, 0, 0)
    return lt_ptr, pi_ptr, lm_ptr, k_ptr, plt_ptr, n_ptr, lists[0].shape[0] if lists is not None else 0


class _ResidentDecoder:
    """``viterbi``'s decode of a log observation table that is already on the device in the kernel's layout [chain][step][state] (``pyin``'s
    observation stage writes it there): the tables of ``viterbi(prob, transition, p_init=p_init, transition_min_prob=...)`` for float64 ``prob``
    built once on the host, every check before device work; ``run`` uploads them into a session and launches ``lra_viterbi_exec`` alone."""

    def __init__(self, transition, p_init, transition_min_prob):
        n_states = int(transition.shape[0])
        _check_states(n_states)
        _check_transition(transition, n_states)
        epsilon = tiny(np.empty(0, dtype=np.float64))
        p_init = _check_p_init(p_init, n_states)
        self.n_states = n_states
        self.threshold = _threshold(transition_min_prob, epsilon)
        self.log_trans, self.log_p_init, self.lists = _search_tables(np.log(transition + epsilon)[None], np.log(p_init + epsilon)[None], self.threshold, n_states)
        if self.lists is not None:
            self.log_trans = None   # (the lists carry every entry the search reads)

    def run(self, sess, log_prob_ptr, ptr_ptr, chains, n_steps):
        """Returns the handle of the states (chains, n_steps) uint16; ``ptr_ptr``: 2 bytes per chain, step and state of scratch."""
        lt_ptr, pi_ptr, _, k_ptr, plt_ptr, n_ptr, n_pred = _upload_tables(sess, self.log_trans, self.log_p_init, None, self.lists)
        states_ptr, states_h = sess.output((chains, n_steps), np.uint16)
        logp_ptr = sess.scratch(8 * max(chains, 1))
        sess.ctx.viterbi_exec(log_prob_ptr, chains, self.n_states, n_steps, lt_ptr, pi_ptr, 1, float(self.threshold), n_pred, k_ptr, plt_ptr, n_ptr, ptr_ptr, states_ptr, logp_ptr)
        return states_ptr, states_h


def _decode(x, kind, real, epsilon, n_states, n_steps, chains, log_trans, log_p_init, log_marginal, threshold, n_labels, flag_check):
    """x: (chains, n_states, n_steps) (binary: (chains, n_steps)) array or tensor of ``real``; the tables float64 on the host: log_trans
    (n_tables, n_states, n_states), log_p_init (n_tables, n_states).  Returns states (chains, n_steps) uint16 and logp (chains,) float64."""
    log_trans, log_p_init, lists = _search_tables(log_trans, log_p_init, threshold, n_states)
    n_tables = log_trans.shape[0]
    if n_steps < 1:
        raise ParameterError(f"prob must hold at least one step, given n_steps={n_steps}")
    sess = _arrays.Session(x)
    try:
        ctx = sess.ctx
        lt_ptr, pi_ptr, lm_ptr, k_ptr, plt_ptr, n_ptr, n_pred = _upload_tables(sess, log_trans, log_p_init, log_marginal, lists)
        states_ptr, states_h = sess.output((chains, n_steps), np.uint16)
        logp_ptr, logp_h = sess.output((chains,), np.float64)
        per_chain = 10 * n_states * n_steps
        chunk = int(max(1, min(chains, SCRATCH_BUDGET // per_chain))) if chains else 0
        if kind == ctx.VITERBI_BINARY:   # (whole items of the batch: a chunk starts at label 0)
            chunk = max(n_labels, chunk // n_labels * n_labels)
        work = sess.scratch(16)
        if chains:
            lp_ptr = sess.scratch(8 * chunk * n_states * n_steps)
            ptr_ptr = sess.scratch(2 * chunk * n_states * n_steps)
        for c0 in range(0, chains, chunk or 1):
            c1 = min(chains, c0 + chunk)
            x_ptr = sess.input_raw(x[c0:c1], real)
            flags = ctx.viterbi_prep_exec(x_ptr, real, kind, c1 - c0, n_states, n_steps, float(epsilon), lm_ptr, n_labels, lp_ptr, work)
            flag_check(flags, ctx)
            ctx.viterbi_exec(lp_ptr, c1 - c0, n_states, n_steps, lt_ptr, pi_ptr, n_tables, float(threshold), n_pred, k_ptr, plt_ptr, n_ptr, ptr_ptr, states_ptr + 2 * c0 * n_steps,
                             logp_ptr + 8 * c0)
        return sess.result(states_h), sess.result(logp_h)
    finally:
        sess.close()


def _as_like(sess, a):
    """A host table as the session's kind of array (a tensor on the session's device for tensor callers)."""
    if not sess.is_torch:
        return a
    import torch

    if a.dtype == np.uint16:   # (uploaded through its bits: not every torch build copies uint16 from NumPy)
        return torch.from_numpy(a.view(np.int16)).to(sess.device).view(torch.uint16)
    return torch.from_numpy(a).to(sess.device)


def _flat(prob, keep):
    """prob with its leading dimensions folded into one: (chains, *last `keep` dims)."""
    tail = tuple(int(s) for s in prob.shape[prob.ndim - keep:])
    return prob.reshape((-1,) + tail), tuple(int(s) for s in prob.shape[:prob.ndim - keep])


def _no_flags(flags, ctx):
    return None


def _viterbi_log(log_prob, log_trans, log_p_init, log_trans_threshold):
    """``_viterbi`` (``librosa/sequence.py:1174-1259``) of float64 log tables as given, on the device: ``log_prob`` of shape
    ``(..., n_states, n_steps)``, ``log_trans`` ``(n_states, n_states)``, ``log_p_init`` ``(n_states,)``.  Returns the states ``(..., n_steps)``
    (uint16) and ``logp`` ``(..., 1)`` (float64).  Given the reference's tables, the reference's bits."""
    n_states, n_steps = (int(s) for s in log_prob.shape[-2:])
    _check_states(n_states)
    log_trans = _host(log_trans)
    log_p_init = _host(log_p_init)
    if log_trans.shape != (n_states, n_states) or log_p_init.shape != (n_states,):
        raise ParameterError(f"log_trans.shape={log_trans.shape} and log_p_init.shape={log_p_init.shape} must be (n_states, n_states) and (n_states,) for n_states={n_states}")
    x, lead = _flat(_arrays.cast(log_prob, np.float64), 2)
    ctx_kind = _native.Context.VITERBI_LOG
    states, logp = _decode(x, ctx_kind, np.dtype(np.float64), 0.0, n_states, n_steps, int(x.shape[0]), log_trans[None], log_p_init[None], None, float(log_trans_threshold), 1, _no_flags)
    return states.reshape(lead + (n_steps,)), logp.reshape(lead + (1,))


def _check_transition(transition, n_states):
    if transition.shape != (n_states, n_states):
        raise ParameterError(f"transition.shape={transition.shape}, must be (n_states, n_states)={n_states, n_states}")
    if np.any(transition < 0) or not np.allclose(transition.sum(axis=1), 1):
        raise ParameterError("Invalid transition matrix: must be non-negative and sum to 1 on each row.")


def _check_p_init(p_init, n_states):
    if p_init is None:
        p_init = np.empty(n_states)
        p_init.fill(1.0 / n_states)
        return p_init
    p_init = _host(p_init)
    if np.any(p_init < 0) or not np.allclose(p_init.sum(), 1) or p_init.shape != (n_states,):
        raise ParameterError(f"Invalid initial state distribution: p_init={p_init}")
    return p_init


def _finish(states, logp, lead, n_steps, return_logp, squeeze_2d):
    """The reference's return shapes: a 2-D call gives logp of shape (1,) (``squeeze_2d`` false) or a scalar; a batch gives logp of the lead shape."""
    states = states.reshape(lead + (n_steps,))
    if not return_logp:
        return states
    if lead or squeeze_2d:
        return states, logp.reshape(lead)
    return states, logp.reshape((1,))


def viterbi(prob, transition, *, p_init=None, return_logp=False, transition_min_prob=None):
    """Viterbi decoding from observation likelihoods (``librosa/sequence.py:1280-1432``).

    ``prob`` of shape ``(..., n_states, n_steps)``: a NumPy array, or a tensor on the device (then the results are tensors there).  Returns
    the states ``(..., n_steps)`` (uint16) and, with ``return_logp``, their log probability (float64; shape ``(1,)`` for a 2-D ``prob``)."""
    n_states, n_steps = (int(s) for s in prob.shape[-2:])
    _check_states(n_states)
    transition = _host(transition)
    _check_transition(transition, n_states)
    prob, real, epsilon = _as_real(prob)
    p_init = _check_p_init(p_init, n_states)
    log_trans = np.log(transition + epsilon)
    log_p_init = np.log(p_init + epsilon)
    threshold = _threshold(transition_min_prob, epsilon)

    def check(flags, ctx):
        if flags & (ctx.VITERBI_FLAG_NEGATIVE | ctx.VITERBI_FLAG_ABOVE_ONE):
            raise ParameterError("Invalid probability values: must be between 0 and 1.")

    x, lead = _flat(prob, 2)
    states, logp = _decode(x, _native.Context.VITERBI_GENERATIVE, real, epsilon, n_states, n_steps, int(x.shape[0]), log_trans[None], log_p_init[None], None, threshold, 1, check)
    return _finish(states, logp, lead, n_steps, return_logp, False)


def viterbi_discriminative(prob, transition, *, p_state=None, p_init=None, return_logp=False, transition_min_prob=None):
    """Viterbi decoding from discriminative state predictions (``librosa/sequence.py:1455-1679``); ``logp`` is a scalar for a 2-D ``prob``."""
    n_states, n_steps = (int(s) for s in prob.shape[-2:])
    _check_states(n_states)
    transition = _host(transition)
    _check_transition(transition, n_states)
    prob, real, epsilon = _as_real(prob)
    if p_state is None:
        p_state = np.empty(n_states)
        p_state.fill(1.0 / n_states)
    else:
        p_state = _host(p_state)
        if p_state.shape != (n_states,):
            raise ParameterError(f"Marginal distribution p_state must have shape (n_states,). Got p_state.shape={p_state.shape}")
        if np.any(p_state < 0) or not np.allclose(p_state.sum(axis=-1), 1):
            raise ParameterError(f"Invalid marginal state distribution: p_state={p_state}")
    p_init = _check_p_init(p_init, n_states)
    log_p_init = np.log(p_init + epsilon)
    log_trans = np.log(transition + epsilon)
    log_marginal = np.log(p_state + epsilon)
    threshold = _threshold(transition_min_prob, epsilon)

    def check(flags, ctx):
        if flags & (ctx.VITERBI_FLAG_NEGATIVE | ctx.VITERBI_FLAG_COLUMN_SUM):
            raise ParameterError("Invalid probability values: each column must sum to 1 and be non-negative")

    x, lead = _flat(prob, 2)
    states, logp = _decode(x, _native.Context.VITERBI_DISCRIMINATIVE, real, epsilon, n_states, n_steps, int(x.shape[0]), log_trans[None], log_p_init[None], log_marginal, threshold, 1,
                           check)
    return _finish(states, logp, lead, n_steps, return_logp, True)


def viterbi_binary(prob, transition, *, p_state=None, p_init=None, return_logp=False, transition_min_prob=None):
    """Viterbi decoding from binary (multi-label) state predictions (``librosa/sequence.py:1702-1874``): every label of every item is a 2-state
    chain with its own table, initial and marginal distribution, and all of them are decoded in one launch."""
    if prob.ndim < 2:
        prob = prob.reshape((1,) * (2 - prob.ndim) + tuple(prob.shape))
    n_states, n_steps = (int(s) for s in prob.shape[-2:])
    transition = _host(transition)
    if transition.shape == (2, 2):
        transition = np.tile(transition, (n_states, 1, 1))
    elif transition.shape != (n_states, 2, 2):
        raise ParameterError(f"transition.shape={transition.shape}, must be (2, 2) or (n_states, 2, 2)={n_states}")
    if np.any(transition < 0) or not np.allclose(transition.sum(axis=-1), 1):
        raise ParameterError("Invalid transition matrix: must be non-negative and sum to 1 on each row.")
    prob, real, _ = _as_real(prob)
    if p_state is None:
        p_state = np.empty(n_states)
        p_state.fill(0.5)
    else:
        p_state = np.atleast_1d(_host(p_state))
    if p_state.shape != (n_states,) or np.any(p_state < 0) or np.any(p_state > 1):
        raise ParameterError(f"Invalid marginal state distributions: p_state={p_state}")
    if p_init is None:
        p_init = np.empty(n_states)
        p_init.fill(0.5)
    else:
        p_init = np.atleast_1d(_host(p_init))
    if p_init.shape != (n_states,) or np.any(p_init < 0) or np.any(p_init > 1):
        raise ParameterError(f"Invalid initial state distributions: p_init={p_init}")
    # each label's call of viterbi_discriminative on float64 rows (:1848-1869): epsilon is float64's whatever prob's type
    epsilon = tiny(np.empty(0, dtype=np.float64))
    threshold = _threshold(transition_min_prob, epsilon)
    pair = lambda p: np.stack([(1 - p).astype(np.float64), p.astype(np.float64)], axis=-1)   # (label, 2): p_*_binary of every label (1 - p in p's own type, :1856-1860)
    log_p_init = np.log(pair(p_init) + epsilon)
    log_marginal = np.log(pair(p_state) + epsilon)
    log_trans = np.log(transition + epsilon)

    def check(flags, ctx):
        if flags & (ctx.VITERBI_FLAG_NEGATIVE | ctx.VITERBI_FLAG_ABOVE_ONE):
            raise ParameterError("Invalid probability values: prob must be between [0, 1]")

    x, lead = _flat(prob, 1)   # (items * labels, n_steps): chain c is label c % n_states
    states, logp = _decode(x, _native.Context.VITERBI_BINARY, real, epsilon, 2, n_steps, int(x.shape[0]), log_trans, log_p_init, log_marginal, threshold, n_states, check)
    states = states.reshape(lead + (n_steps,))
    if return_logp:
        return states, logp.reshape(lead)
    return states


def transition_uniform(n_states):
    """``librosa/sequence.py:1877-1902``."""
    if not is_positive_int(n_states):
        raise ParameterError(f"n_states={n_states} must be a positive integer")
    transition = np.empty((n_states, n_states), dtype=np.float64)
    transition.fill(1.0 / n_states)
    return transition


def _self_prob(n_states, prob):
    prob = np.asarray(prob, dtype=np.float64)
    if prob.ndim == 0:
        prob = np.tile(prob, n_states)
    if prob.shape != (n_states,):
        raise ParameterError(f"prob={prob} must have length equal to n_states={n_states}")
    if np.any(prob < 0) or np.any(prob > 1):
        raise ParameterError(f"prob={prob} must have values in the range [0, 1]")
    return prob


def transition_loop(n_states, prob):
    """``librosa/sequence.py:1905-1967``."""
    if not (is_positive_int(n_states) and (n_states > 1)):
        raise ParameterError(f"n_states={n_states} must be a positive integer > 1")
    transition = np.empty((n_states, n_states), dtype=np.float64)
    for i, prob_i in enumerate(_self_prob(n_states, prob)):
        transition[i] = (1.0 - prob_i) / (n_states - 1)
        transition[i, i] = prob_i
    return transition


def transition_cycle(n_states, prob):
    """``librosa/sequence.py:1970-2031``."""
    if not (is_positive_int(n_states) and n_states > 1):
        raise ParameterError(f"n_states={n_states} must be a positive integer > 1")
    transition = np.zeros((n_states, n_states), dtype=np.float64)
    for i, prob_i in enumerate(_self_prob(n_states, prob)):
        transition[i, np.mod(i + 1, n_states)] = 1.0 - prob_i
        transition[i, i] = prob_i
    return transition


def transition_local(n_states, width, *, window="triangle", wrap=False):
    """``librosa/sequence.py:2034-2146``."""
    if not (is_positive_int(n_states) and n_states > 1):
        raise ParameterError(f"n_states={n_states} must be a positive integer > 1")
    width = np.asarray(width, dtype=int)
    if width.ndim == 0:
        width = np.tile(width, n_states)
    if width.shape != (n_states,):
        raise ParameterError(f"width={width} must have length equal to n_states={n_states}")
    if np.any(width < 1):
        raise ParameterError(f"width={width} must be at least 1")
    transition = np.zeros((n_states, n_states), dtype=np.float64)
    for i, width_i in enumerate(width):
        trans_row = pad_center(get_window(window, width_i, fftbins=False), size=n_states)
        trans_row = np.roll(trans_row, n_states // 2 + i + 1)
        if not wrap:
            trans_row[min(n_states, i + width_i // 2 + 1):] = 0
            trans_row[: max(0, i - width_i // 2)] = 0
        transition[i] = trans_row
    transition /= transition.sum(axis=1, keepdims=True)
    return transition


# ---- dynamic time warping (librosa/sequence.py:185-694) -----------------------------------------------------------------------------------------
DTW_MAX_STEPS = 16           # LRA_DTW_MAX_STEPS: rows of the step table, the three defaults included
DTW_MAX_STEP = 8             # LRA_DTW_MAX_STEP: the largest step component
DTW_METRICS = ("euclidean", "sqeuclidean", "cityblock", "cosine")
DTW_TILE = 0                 # the accumulate kernel's tile edge: 0 for the library's choice, or 8, 16, 32, 64 (tests reach many-tile grids at tiny shapes)
_CDIST_TEXT = ("scipy.spatial.distance.cdist returned an error.\n"
               "Please provide your input in the form X.shape=(K, N) "
               "and Y.shape=(K, M).\n 1-dimensional sequences should "
               "be reshaped to X.shape=(1, N) and Y.shape=(1, M).")
_NO_PATH_TEXT = "No valid sub-sequence warping path could be constructed with the given step sizes."


def _dtw_default_steps():
    return np.array([[1, 1], [0, 1], [1, 0]], dtype=np.uint32)


def _dtw_device_limits(step_sizes_sigma):
    """The documented differences of the step table: the int64 table the kernels take, or ParameterError."""
    steps = np.asarray(step_sizes_sigma)
    if steps.ndim != 2 or steps.shape[1] != 2 or np.any(steps != np.floor(steps)):
        raise ParameterError(f"step_sizes_sigma must be an integer array of shape (n, 2), given shape {steps.shape}")
    steps = steps.astype(np.int64)
    if np.any((steps == 0).all(axis=1)):
        raise ParameterError("step_sizes_sigma cannot contain the step (0, 0): the device's wavefront has no order for it")
    if len(steps) > DTW_MAX_STEPS:
        raise ParameterError(f"step_sizes_sigma holds {len(steps)} steps with the three defaults: at most {DTW_MAX_STEPS} are served")
    if steps.max() > DTW_MAX_STEP:
        raise ParameterError(f"step_sizes_sigma holds a step component of {int(steps.max())}: at most {DTW_MAX_STEP} is served")
    return steps


def _atleast_2d(a):
    if is_torch_tensor(a):
        return a.reshape((1,) * (2 - a.ndim) + tuple(a.shape)) if a.ndim < 2 else a
    return np.atleast_2d(a)


def _same_kind(sess, a):
    """``a`` as the session's kind of array."""
    if sess.is_torch:
        return a.to(sess.device) if is_torch_tensor(a) else _as_like(sess, np.ascontiguousarray(a))
    return _host(a)


def _dtw_features(X):
    """(..., K, N) -> (features, N) in ``X.reshape(-1, N)``'s order, float32 or float64."""
    X = _atleast_2d(X)
    n = int(X.shape[-1])
    X = X.reshape((-1, n))
    return X if np.dtype(_arrays.numpy_dtype_of(X)) in (np.dtype(np.float32), np.dtype(np.float64)) else _arrays.cast(X, np.float64)


def dtw(X=None, Y=None, *, C=None, metric="euclidean", step_sizes_sigma=None, weights_add=None, weights_mul=None, subseq=False, backtrack=True, global_constraints=False, band_rad=0.25,
        return_steps=False):
    """Dynamic time warping (``librosa/sequence.py:185-498``): the cost matrix of ``X`` (..., K, N) and ``Y`` (..., K, M) (or a given ``C``), the
    accumulated cost matrix ``D`` (float64), the warping path ``wp`` (int64, (L, 2); with ``backtrack``) and the step matrix ``steps`` (int32; with
    ``return_steps``), all computed on the device.  NumPy input gives NumPy results, tensors on the device give tensors there; the input is never
    written.  Differences from the reference: the module docstring."""
    default_steps = _dtw_default_steps()
    default_weights_add = np.zeros(3, dtype=np.float64)
    default_weights_mul = np.ones(3, dtype=np.float64)
    if step_sizes_sigma is None:
        step_sizes_sigma = default_steps
        if weights_add is None:
            weights_add = default_weights_add
        if weights_mul is None:
            weights_mul = default_weights_mul
    else:
        step_sizes_sigma = _host(step_sizes_sigma)
        if weights_add is None:
            weights_add = np.zeros(len(step_sizes_sigma), dtype=np.float64)
        if weights_mul is None:
            weights_mul = np.ones(len(step_sizes_sigma), dtype=np.float64)
        # the defaults get infinite weights (inf * 0.0 is NaN and loses every <, as on the host)
        default_weights_add.fill(np.inf)
        default_weights_mul.fill(np.inf)
        step_sizes_sigma = np.concatenate((default_steps, step_sizes_sigma))
        weights_add = np.concatenate((default_weights_add, _host(weights_add)))
        weights_mul = np.concatenate((default_weights_mul, _host(weights_mul)))
    weights_add, weights_mul = _host(weights_add), _host(weights_mul)

    if np.any(step_sizes_sigma < 0):
        raise ParameterError("step_sizes_sigma cannot contain negative values")
    if len(step_sizes_sigma) != len(weights_add):
        raise ParameterError("len(weights_add) must be equal to len(step_sizes_sigma)")
    if len(step_sizes_sigma) != len(weights_mul):
        raise ParameterError("len(weights_mul) must be equal to len(step_sizes_sigma)")
    if C is None and (X is None or Y is None):
        raise ParameterError("If C is not supplied, both X and Y must be supplied")
    if C is not None and (X is not None or Y is not None):
        raise ParameterError("If C is supplied, both X and Y must not be supplied")
    steps_table = _dtw_device_limits(step_sizes_sigma)

    c_is_transposed = False
    if C is None:
        if metric not in DTW_METRICS:
            raise ParameterError(f"metric={metric!r} is not served on the device: one of {', '.join(DTW_METRICS)}")
        X, Y = _dtw_features(X), _dtw_features(Y)
        if int(X.shape[0]) != int(Y.shape[0]):
            raise ParameterError(_CDIST_TEXT)
        if subseq and int(X.shape[1]) > int(Y.shape[1]):
            X, Y = Y, X   # C.T: every metric served gives the same bits with its arguments exchanged
            c_is_transposed = True
        n, m = int(X.shape[1]), int(Y.shape[1])
        like = X if is_torch_tensor(X) or not is_torch_tensor(Y) else Y
    else:
        C = _atleast_2d(C)
        if C.ndim != 2:
            raise ParameterError(f"C must be a matrix, given shape {tuple(C.shape)}")
        n, m = int(C.shape[0]), int(C.shape[1])
        like = C
    if n < 1 or m < 1:
        raise ParameterError(f"the cost matrix is empty: shape {(n, m)}")

    # (the reference compares the concatenated table, so this practically never fires; kept where it is)
    if np.array_equal(step_sizes_sigma, np.array([[1, 1]])) and n > m:
        raise ParameterError("For diagonal matching: Y.shape[-1] >= X.shape[-11] (C.shape[1] >= C.shape[0])")

    band = None
    if global_constraints:
        # util.fill_off_diagonal's rule (util/utils.py:2050-2067), applied as a predicate where C is read
        radius = int(np.round(band_rad * min(n, m)))
        offset = abs(n - m)
        band = (-radius, radius + offset) if n < m else (-radius - offset, radius)

    sess = _arrays.Session(like)
    try:
        ctx = sess.ctx
        work = sess.scratch(16)
        if C is None:
            real = np.dtype(np.float32) if all(np.dtype(_arrays.numpy_dtype_of(a)) == np.float32 for a in (X, Y)) else np.dtype(np.float64)
            x_ptr = sess.input_raw(_same_kind(sess, X), real)
            y_ptr = sess.input_raw(_same_kind(sess, Y), real)
            c_ptr = sess.scratch(8 * n * m)
            flags = ctx.dtw_cost_exec(x_ptr, y_ptr, real, int(X.shape[0]), n, m, ctx.DTW_METRICS[metric], c_ptr, work)
        else:
            np_dtype = np.dtype(_arrays.numpy_dtype_of(C))
            if np_dtype.name not in ctx.DTW_TYPES:
                if np_dtype.kind not in "biuf":
                    raise ParameterError(f"C must be real-valued, given dtype={np_dtype}")
                C, np_dtype = _arrays.cast(C, np.float64), np.dtype(np.float64)
            in_ptr = sess.input_raw(C, np_dtype)
            c_ptr = in_ptr if np_dtype == np.float64 else sess.scratch(8 * n * m)   # (a float64 C is read where it lies)
            flags = ctx.dtw_prepare_exec(in_ptr, np_dtype, n * m, 0 if np_dtype == np.float64 else c_ptr, work)
        if flags & ctx.DTW_FLAG_NAN:
            raise ParameterError("DTW cost matrix C has NaN values. ")

        d_ptr, d_h = sess.output((n, m), np.float64)
        idx_ptr = sess.scratch(n * m)
        ctx.dtw_accumulate_exec(c_ptr, n, m, steps_table, weights_add, weights_mul, subseq, band, DTW_TILE, d_ptr, idx_ptr)

        wp = None
        if backtrack:
            path_ptr, path_h = sess.output((n + m - 1, 2), np.int64)
            length, status = ctx.dtw_backtrack_exec(d_ptr, idx_ptr, False, n, m, steps_table, subseq, ctx.DTW_START_ARGMIN if subseq else ctx.DTW_START_END, path_ptr, work)
            if status & (ctx.DTW_FLAG_ROW_INF | ctx.DTW_FLAG_END_INF):
                raise ParameterError(_NO_PATH_TEXT)
            if status & ctx.DTW_FLAG_NOT_ORIGIN:
                raise ParameterError("Unable to compute a full DTW warping path. You may want to try again with subseq=True.")
            wp = sess.result(path_h)[:length]
            # the reference's three conditions for flipping the pairs back (:480-485): X longer than Y, or a given C with more rows than columns
            if subseq and (c_is_transposed or n > m):
                wp = wp.flip(1) if sess.is_torch else np.fliplr(wp)
        steps = None
        if return_steps:
            steps_ptr, steps_h = sess.output((n, m), np.int32)
            ctx.dtw_widen_exec(idx_ptr, n * m, steps_ptr)
            steps = sess.result(steps_h)
        out = [sess.result(d_h)] + ([wp] if backtrack else []) + ([steps] if return_steps else [])
        return tuple(out) if len(out) > 1 else out[0]
    finally:
        sess.close()


def dtw_backtracking(steps, *, step_sizes_sigma=None, subseq=False, start=None):
    """Backtrack a warping path from a step matrix (``librosa/sequence.py:643-694``), on the device: ``wp`` int64 (L, 2), a tensor where ``steps``
    is one.  An index of ``steps`` outside the step table raises ``ParameterError`` (the reference: ``IndexError``)."""
    if subseq is False and start is not None:
        raise ParameterError(f"start is only allowed to be set if subseq is True (start={start}, subseq={subseq})")
    default_steps = _dtw_default_steps()
    if step_sizes_sigma is None:
        step_sizes_sigma = default_steps
    else:
        step_sizes_sigma = np.concatenate((default_steps, _host(step_sizes_sigma)))
    if np.any(step_sizes_sigma < 0):
        raise ParameterError("step_sizes_sigma cannot contain negative values")
    steps_table = _dtw_device_limits(step_sizes_sigma)
    if steps.ndim != 2 or int(steps.shape[0]) < 1 or int(steps.shape[1]) < 1:
        raise ParameterError(f"steps must be a non-empty matrix, given shape {tuple(steps.shape)}")
    n, m = int(steps.shape[0]), int(steps.shape[1])
    if start is not None and not 0 <= int(start) < m:
        raise ParameterError(f"start={start} is not a column of steps (shape {(n, m)})")
    sess = _arrays.Session(steps)
    try:
        ctx = sess.ctx
        idx_ptr = sess.input_raw(steps, np.int32)
        path_ptr, path_h = sess.output((n + m - 1, 2), np.int64)
        length, status = ctx.dtw_backtrack_exec(0, idx_ptr, True, n, m, steps_table, subseq, ctx.DTW_START_END if start is None else int(start), path_ptr, sess.scratch(16))
        if status & ctx.DTW_FLAG_BAD_STEP:
            raise ParameterError(f"steps holds an index outside the step table of {len(steps_table)} steps")
        return sess.result(path_h)[:length]
    finally:
        sess.close()


# ---- recurrence quantification analysis (librosa/sequence.py:698-1074) --------------------------------------------------------------------------
RQA_ROWS = 0                 # the scoring kernel's rows per launch: 0 for the library's choice, or a power of two up to 64
RQA_STRIP = 0                # its columns per workgroup: 0 for the library's choice, or a power of two from 4 to 1024 (tests reach many launches and strips at tiny shapes)


def rqa(sim, *, gap_onset=1, gap_extend=1, knight_moves=True, backtrack=True):
    """Recurrence quantification analysis (``librosa/sequence.py:698-1074``): the alignment score matrix ``score`` of a self- or cross-similarity
    matrix ``sim`` (N, M), in ``sim``'s type for float32 and float64 (float64 for bool and integer ``sim``), and with ``backtrack`` the best
    alignment ``path`` (uint64, (k, 2), ascending; (0, 2) where nothing aligns), all computed on the device.  NumPy input gives NumPy results, a
    tensor on the device gives tensors there; the input is never written.  Differences from the reference: the module docstring."""
    if gap_onset < 0:
        raise ParameterError("gap_onset={} must be strictly positive")
    if gap_extend < 0:
        raise ParameterError("gap_extend={} must be strictly positive")
    if not (is_torch_tensor(sim) or isinstance(sim, np.ndarray)):
        sim = np.asarray(sim)
    if sim.ndim != 2:
        raise ParameterError(f"sim must be a matrix, given shape {tuple(sim.shape)}")
    n, m = int(sim.shape[0]), int(sim.shape[1])
    if n < 1 or m < 1:
        raise ParameterError(f"sim is empty: shape {(n, m)}")
    if is_torch_tensor(sim):
        import torch

        if sim.dtype == torch.bool:
            sim = sim.view(torch.uint8)
        elif sim.is_complex():
            raise ParameterError(f"sim must be real-valued, given dtype={sim.dtype}")
    elif sim.dtype == np.bool_:
        sim = sim.view(np.uint8)
    np_dtype = np.dtype(_arrays.numpy_dtype_of(sim))
    if np_dtype.kind not in "iuf":
        raise ParameterError(f"sim must be real-valued, given dtype={np_dtype}")
    widen = np_dtype.name in ("uint8", "int32", "int64")   # (exactly, on the device: dtw_prepare)
    if np_dtype not in (np.dtype(np.float32), np.dtype(np.float64)) and not widen:
        sim, np_dtype = _arrays.cast(sim, np.float64), np.dtype(np.float64)
    real = np.dtype(np.float64) if widen else np_dtype

    sess = _arrays.Session(sim)
    try:
        ctx = sess.ctx
        sim_ptr = sess.input_raw(sim, np_dtype)
        if widen:
            in_ptr, sim_ptr = sim_ptr, sess.scratch(8 * n * m)
            ctx.dtw_prepare_exec(in_ptr, np_dtype, n * m, sim_ptr, sess.scratch(16))   # (its NaN flag: an integer holds none)
        score_ptr, score_h = sess.output((n, m), real)
        ptr_ptr = sess.scratch(n * m)
        ctx.rqa_score_exec(sim_ptr, real, n, m, gap_onset, gap_extend, knight_moves, RQA_ROWS, RQA_STRIP, score_ptr, ptr_ptr)
        if not backtrack:
            return sess.result(score_h)
        cap = min(n, m)
        # (allocated as int64 and viewed as uint64: not every torch build slices or copies uint64 on the device)
        path_ptr, path_h = sess.output((cap, 2), np.int64)
        work = sess.scratch(ctx.RQA_WORK_BYTES)
        ctx.rqa_argmax_exec(score_ptr, real, n * m, work)
        length = ctx.rqa_backtrack_exec(ptr_ptr, n, m, work, path_ptr)
        path = sess.result(path_h)[cap - length:]
        path = path.view(_arrays.torch_dtype(np.uint64)) if sess.is_torch else path.view(np.uint64)
        return sess.result(score_h), path
    finally:
        sess.close()
