"""Sequence decoding: ``librosa.sequence``'s Viterbi decoders and transition builders (``librosa/sequence.py:1174-2146``).

``viterbi``, ``viterbi_discriminative`` and ``viterbi_binary`` have the reference's signatures, checks and messages.  The small float64 tables
(``log_trans``, ``log_p_init``, ``log_marginal``, the threshold and the predecessor lists) are built here with NumPy, bit-equal to the
reference's; the signal-sized ``log_prob`` is computed on the device (``csrc/lra_viterbi.h``: ``viterbi_prep``), which also raises the range
flags on ``prob`` that are read before the decode is launched.  Every sequence of a batch is decoded in one launch: a workgroup per sequence
(``viterbi_wg``), or a group of lanes per chain up to 32 states (``viterbi_small``: all labels of ``viterbi_binary`` at once).

Differences from the reference: ``n_states`` above ``MAX_STATES`` raises ``ParameterError`` (a sequence's two value rows live
in the LDS of one workgroup); ``prob`` must be float32 or float64 (other types are converted as NumPy's promotion with ``tiny(prob)`` would);
a float32 ``p_state`` is widened before it is subtracted.
"""
from __future__ import annotations

import numpy as np

from . import _arrays, _native
from .filters import get_window
from .util.exceptions import ParameterError
from .util.utils import is_positive_int, is_torch_tensor, pad_center, tiny

__all__ = ["viterbi", "viterbi_discriminative", "viterbi_binary", "transition_uniform", "transition_loop", "transition_cycle", "transition_local"]

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
