"""Feature manipulation: ``stack_memory`` (``librosa/feature/utils.py:134-314``), one gather launch on the device (``csrc/lra_enhance.h``:
enhance_stack).  The pad of the reference is an index map there: nothing padded is allocated."""
from __future__ import annotations

import numpy as np

from .. import _arrays
from ..util.exceptions import ParameterError
from ..util.utils import is_torch_tensor

__all__ = ["stack_memory"]

_PAD_MODES = ("constant", "edge", "reflect", "symmetric", "wrap")


def _fill_bits(value, x):
    """The bytes of ``constant_values`` in the type of ``x``, as an unsigned integer."""
    if np.ndim(value) != 0:
        value = np.asarray(value)
        if value.size != 1:
            raise ParameterError(f"stack_memory: constant_values must be a scalar on the device, given shape={value.shape}")
        value = value.reshape(())[()]
    if is_torch_tensor(x):
        one = _arrays._torch().full((1,), value, dtype=x.dtype).view(_arrays._torch().uint8).numpy()
    else:
        one = np.asarray(value).astype(x.dtype).reshape(1).view(np.uint8)
    return int.from_bytes(one.tobytes(), "little")


def stack_memory(data, *, n_steps=2, delay=1, **kwargs):
    """Short-term history embedding: ``data`` ``(..., d, t)`` stacked with ``n_steps - 1`` copies of itself delayed by multiples of ``delay``
    columns, shape ``(..., d * n_steps, t)``, type kept.  Columns before the start (after the end for a negative ``delay``) come from
    ``np.pad``'s ``mode``: ``constant`` (a scalar ``constant_values``, default 0), ``edge``, ``reflect``, ``symmetric`` or ``wrap``; any other
    keyword argument of ``np.pad`` raises ``ParameterError``.  NumPy in gives NumPy out, a device tensor gives a device tensor."""
    if n_steps < 1:
        raise ParameterError("n_steps must be a positive integer")
    if delay == 0:
        raise ParameterError("delay must be a non-zero integer")
    if not (is_torch_tensor(data) or isinstance(data, np.ndarray)):
        data = np.asarray(data)
    if data.ndim < 2:
        data = data.reshape((1, -1)) if data.ndim == 1 else data.reshape((1, 1))
    shape = tuple(int(s) for s in data.shape)
    t = shape[-1]
    if t < 1:
        raise ParameterError(f"Cannot stack memory when input data has no columns. Given data.shape={shape}")
    for key in kwargs:
        if key not in ("mode", "constant_values"):
            raise ParameterError(f"stack_memory: the keyword argument {key!r} of np.pad is not served on the device (mode and constant_values are)")
    mode = kwargs.get("mode", "constant")
    if not isinstance(mode, str) or mode not in _PAD_MODES:
        raise ParameterError(f"stack_memory: mode={mode!r} is not served on the device: one of {', '.join(_PAD_MODES)}")
    if "constant_values" in kwargs and mode != "constant":
        raise ParameterError(f"stack_memory: constant_values goes with mode='constant', given mode={mode!r}")
    fill = _fill_bits(kwargs.get("constant_values", 0), data) if mode == "constant" else 0
    n_steps, delay = int(n_steps), int(delay)
    d = shape[-2]
    batch = int(np.prod(shape[:-2], dtype=np.int64))
    out_shape = shape[:-2] + (d * n_steps, t)
    if (data.element_size() if is_torch_tensor(data) else data.dtype.itemsize) not in (1, 2, 4, 8):
        raise ParameterError(f"stack_memory moves elements of 1, 2, 4 or 8 bytes, given dtype={data.dtype}")
    sess = _arrays.Session(data)
    try:
        ptr, esize = sess.input_bytes(data)
        out_ptr, out_h = sess.output_like(out_shape, data)
        if batch * d:
            sess.ctx.stack_memory_exec(ptr, esize, batch, d, t, n_steps, delay, sess.ctx.STACK_MODES[mode], fill, out_ptr)
        return sess.result(out_h)
    finally:
        sess.close()
