"""``peak_pick`` with librosa's signature (``librosa/util/utils.py:1326-1496``) on the device kernels of ``csrc/lra_peaks.h``.

The rows are uploaded once (device tensors are used where they are), three launches run (the row copy with its statistics, the candidate
flags, and the greedy selection or the dynamic program), and one ``uint8`` row per input row comes back.  ``sparse=True`` turns it into
indices (``np.flatnonzero``, or ``torch.nonzero`` for a device tensor).  Device tensors in give device tensors out.

The window maximum, the comparison against it and the dynamic program's sums are the reference's arithmetic bit for bit.  The window mean
is float64 here; the reference rounds it to the row's precision (``np.mean`` for ``greedy``, a ``cumsum`` difference for the ``dp_*``
methods), so the two can differ only at a frame whose ``x[n] - mean - delta`` lies within that rounding.  A NaN in a row: ``greedy`` is the
reference's result; the ``dp_*`` methods differ, because the reference's running sum carries the NaN into every later window and the
device's windows hold only their own frames.  Rows of another dtype than float32 / float64 are picked in float64.
"""
from __future__ import annotations

import numpy as np

from .exceptions import ParameterError
from .utils import is_torch_tensor

# method codes of lra_peak_pick_exec (include/librosa_amd.h)
METHODS = {"greedy": 0, "dp_count": 1, "dp_value": 2}


def _valid_int(x):
    """``valid_int(x, cast=np.ceil)`` (``util/utils.py:311-341``)."""
    return int(np.ceil(x))


def check_ranges(pre_max, post_max, pre_avg, post_avg, delta, wait):
    """``util/utils.py:1428-1439``."""
    if pre_max < 0:
        raise ParameterError("pre_max must be non-negative")
    if pre_avg < 0:
        raise ParameterError("pre_avg must be non-negative")
    if delta < 0:
        raise ParameterError("delta must be non-negative")
    if wait < 0:
        raise ParameterError("wait must be non-negative")
    if post_max <= 0:
        raise ParameterError("post_max must be positive")
    if post_avg <= 0:
        raise ParameterError("post_avg must be positive")


def prepare(*, pre_max, post_max, pre_avg, post_avg, delta, wait, method="greedy"):
    """The range checks, the ceilings (``:1448-1452``) and the method -> the arguments of the device call."""
    check_ranges(pre_max, post_max, pre_avg, post_avg, delta, wait)
    if method not in METHODS:
        raise ParameterError(f"Unknown method {method}")
    return dict(pre_max=_valid_int(pre_max), post_max=_valid_int(post_max), pre_avg=_valid_int(pre_avg), post_avg=_valid_int(post_avg), delta=float(delta), wait=_valid_int(wait),
                method=METHODS[method])


def row_dtype(x):
    """The precision the rows are picked in, or None for an integer / bool array."""
    from .. import _arrays

    dt = _arrays.numpy_dtype_of(x)
    if dt == np.float32:
        return np.dtype(np.float32)
    if dt.kind == "f":
        return np.dtype(np.float64)
    return None


def pick_rows(sess, x_ptr, batch, n, real, params, *, normalize=False, keep_norm=False, status=False):
    """One lra_peak_pick_exec on device rows -> (handle of the uint8 [batch][n] rows, pointer of the normalised rows or None, some entry
    non-zero, every entry finite -- both None unless ``status``, which waits for the stream)."""
    ctx = sess.ctx
    out_ptr, handle = sess.output((batch, n), np.uint8)
    norm_ptr = sess.scratch(max(batch * n, 1) * real.itemsize) if keep_norm else None
    work_ptr = sess.scratch(ctx.peak_pick_work_bytes(batch, n, params["method"]))
    nonzero, finite = ctx.peak_pick_exec(x_ptr, batch, n, real, normalize, params["pre_max"], params["post_max"], params["pre_avg"], params["post_avg"], params["delta"],
                                         params["wait"], params["method"], out_ptr, norm_ptr, work_ptr, status=status)
    return handle, norm_ptr, nonzero, finite


def to_bool(rows):
    return rows != 0 if is_torch_tensor(rows) else rows.astype(bool)


def to_indices(flags):
    """The positions of the True entries of a one-dimensional row, int64."""
    if is_torch_tensor(flags):
        from .. import _arrays

        return _arrays._torch().nonzero(flags).reshape(-1)
    return np.flatnonzero(flags)


def peak_pick(x, *, pre_max, post_max, pre_avg, post_avg, delta, wait, sparse=True, method="greedy", axis=-1):
    """Pick peaks by the three conditions of Boeck et al.; drop-in for ``librosa.util.peak_pick`` (``librosa/util/utils.py:1326-1496``).

    ``x[n]`` is a peak when ``x[n] == max(x[n - pre_max : n + post_max])``, ``x[n] >= mean(x[n - pre_avg : n + post_avg]) + delta`` and the
    last peak lies more than ``wait`` frames back (``greedy``: the earliest frames; ``dp_count`` / ``dp_value``: the most peaks / the largest
    sum of peak values).  ``sparse=True`` (one-dimensional ``x`` only): ``int64`` indices; ``sparse=False``: a bool array of ``x``'s shape.
    Every argument is checked before any device work, in the reference's order."""
    if not is_torch_tensor(x):
        x = np.asarray(x)
    check_ranges(pre_max, post_max, pre_avg, post_avg, delta, wait)
    if sparse and x.ndim != 1:
        raise ParameterError(f"sparse=True (default) does not support {x.ndim}-dimensional inputs. Either set sparse=False or process each dimension independently.")
    params = prepare(pre_max=pre_max, post_max=post_max, pre_avg=pre_avg, post_avg=post_avg, delta=delta, wait=wait, method=method)
    if x.ndim == 0:
        raise ParameterError("peak_pick needs an array of at least one dimension")
    if not -x.ndim <= axis < x.ndim:
        raise ParameterError(f"axis={axis} is out of bounds for an array of dimension {x.ndim}")
    from .. import _arrays

    on_device = is_torch_tensor(x)
    real = row_dtype(x) or np.dtype(np.float64)
    rows = x.swapaxes(axis, -1) if axis not in (-1, x.ndim - 1) else x
    shape = tuple(rows.shape)
    n = int(shape[-1])
    batch = int(np.prod(shape[:-1], dtype=np.int64)) if len(shape) > 1 else 1
    if n == 0 or batch == 0:
        flags = _arrays._torch().zeros(shape, dtype=_arrays._torch().bool, device=x.device) if on_device else np.zeros(shape, dtype=bool)
    else:
        sess = _arrays.Session(x if on_device else np.empty(0))
        try:
            x_ptr = sess.input_raw(rows.reshape(batch, n), real)
            handle, _, _, _ = pick_rows(sess, x_ptr, batch, n, real, params)
            flags = to_bool(sess.result(handle)).reshape(shape)
        finally:
            sess.close()
    if rows is not x:
        flags = flags.swapaxes(axis, -1)
    return to_indices(flags) if sparse else flags
