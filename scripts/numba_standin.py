"""A stand-in ``numba`` module for running the reference's generalised-ufunc kernels as the plain Python they are written in.

TEST INFRASTRUCTURE ONLY (used by ``scripts/make_beat_golden.py``).  ``oracle/ref_shim`` installs its own numba stub only when ``"numba"`` is not
in ``sys.modules`` yet, and that stub's ``guvectorize`` / ``stencil`` raise; ``install()`` here goes first.

``guvectorize`` parses the layout string, resolves the listed type signatures the way a NumPy gufunc does (the first signature to which every
array input casts safely; Python scalars are weak and fit any), allocates the outputs the caller left out in the signature's types (without
signatures the caller must pass every output), loops over the broadcast leading axes and calls the undecorated function body.  A ``()`` input
arrives as a scalar, a ``()`` output as a one-element array.  ``stencil`` covers one-dimensional kernels with offsets -1 .. 1: the body is
evaluated on shifted views of the interior and both ends are zero.  The last call of every kernel is kept in ``LAST`` (name -> outputs).
"""
from __future__ import annotations

import re
import sys
import types

import numpy as np

LAST = {}  # kernel name -> tuple of output arrays of its last call (for the fixtures' diagnostics)


def _parse_layout(layout):
    ins, outs = layout.replace(" ", "").split("->")
    dims = lambda s: [tuple(d for d in g.split(",") if d) for g in re.findall(r"\(([^)]*)\)", s)]  # noqa: E731
    return dims(ins), dims(outs)


def _split_args(inner):
    # "float32[:], float32[:,:], float32" -> top-level commas only
    out, depth, cur = [], 0, ""
    for ch in inner:
        if ch == "[":
            depth += 1
        elif ch == "]":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur)
    return out


def _signature_types(sig):
    """"void(float32[:], float32, int32[:])" -> [dtype, ...] (one per argument, inputs then outputs)."""
    inner = sig[sig.index("(") + 1 : sig.rindex(")")]
    return [np.dtype(t.strip().split("[")[0]) for t in _split_args(inner)]


def guvectorize(*dargs, **dkwargs):
    if len(dargs) == 1:
        sigs, layout = None, dargs[0]
    else:
        sigs, layout = [_signature_types(s) for s in dargs[0]], dargs[1]
    in_dims, out_dims = _parse_layout(layout)
    nin, nout = len(in_dims), len(out_dims)

    def deco(fn):
        def gufunc(*args):
            if len(args) not in (nin, nin + nout):
                raise TypeError(f"{fn.__name__}: expected {nin} inputs and optionally {nout} outputs, got {len(args)} arguments")
            weak = [isinstance(a, (bool, int, float)) for a in args[:nin]]
            inputs = [a if w else np.asarray(a) for a, w in zip(args[:nin], weak)]
            outputs = list(args[nin:])
            types_ = None
            if sigs is not None:
                for cand in sigs:
                    if all(w or np.can_cast(a.dtype, t, "safe") for a, w, t in zip(inputs, weak, cand[:nin])):
                        types_ = cand
                        break
                if types_ is None:
                    raise TypeError(f"{fn.__name__}: no signature matches {[getattr(a, 'dtype', type(a)) for a in inputs]}")
                inputs = [t.type(a) if w else a.astype(t, copy=False) for a, w, t in zip(inputs, weak, types_[:nin])]
            elif not outputs:
                raise TypeError(f"{fn.__name__}: a gufunc without type signatures needs its outputs passed in")
            inputs = [np.asarray(a) for a in inputs]
            # core sizes and the broadcast leading shape
            sizes = {}
            leads = []
            for a, d in zip(inputs, in_dims):
                if a.ndim < len(d):
                    raise ValueError(f"{fn.__name__}: input of shape {a.shape} lacks core dimensions {d}")
                core = a.shape[a.ndim - len(d) :]
                for name, s in zip(d, core):
                    if sizes.setdefault(name, s) != s:
                        raise ValueError(f"{fn.__name__}: core dimension {name} mismatch ({sizes[name]} vs {s})")
                leads.append(a.shape[: a.ndim - len(d)])
            lead = np.broadcast_shapes(*leads)
            given = bool(outputs)
            if not given:
                outputs = [np.empty(lead + tuple(sizes[n] for n in d), dtype=t) for d, t in zip(out_dims, types_[nin:])]
            bins = [np.broadcast_to(a, lead + a.shape[a.ndim - len(d) :]) for a, d in zip(inputs, in_dims)]
            for idx in np.ndindex(*lead):
                call = [b[idx] if d else b[idx][()] for b, d in zip(bins, in_dims)]
                call += [o[idx] if d else o[idx + (np.newaxis,)] for o, d in zip(outputs, out_dims)]
                fn(*call)
            LAST[fn.__name__] = tuple(outputs)
            if given:
                return None
            return outputs[0] if nout == 1 else tuple(outputs)

        gufunc.__name__ = fn.__name__
        gufunc.__wrapped__ = fn
        return gufunc

    return deco


class _Relative:
    """x[k] inside a stencil body: the interior of a 1-D array shifted by k."""

    def __init__(self, x):
        self.x = x

    def __getitem__(self, k):
        if k not in (-1, 0, 1):
            raise IndexError("the stencil stand-in handles offsets -1 .. 1")
        n = len(self.x)
        return self.x[1 + k : n - 1 + k]


def stencil(fn):
    def apply(x):
        x = np.asarray(x)
        if x.ndim != 1:
            raise ValueError("the stencil stand-in handles one-dimensional kernels")
        if len(x) < 3:
            return np.zeros(len(x), dtype=bool)
        inner = np.asarray(fn(_Relative(x)))
        out = np.zeros(len(x), dtype=inner.dtype)
        out[1:-1] = inner
        return out

    apply.__name__ = fn.__name__
    return apply


def _identity(*dargs, **dkwargs):
    if len(dargs) == 1 and callable(dargs[0]) and not dkwargs:
        return dargs[0]
    return lambda fn: fn


def _vectorize(*dargs, **dkwargs):
    def deco(fn):
        nin = fn.__code__.co_argcount

        def ufunc(*args):
            res = fn(*args[:nin])
            if len(args) > nin and args[nin] is not None:
                args[nin][...] = res
                return args[nin]
            return res

        return ufunc

    if len(dargs) == 1 and callable(dargs[0]) and not dkwargs:
        return deco(dargs[0])
    return deco


def install():
    """Put the stand-in into ``sys.modules`` (before the reference is imported)."""
    if "numba" in sys.modules and getattr(sys.modules["numba"], "__version__", "") != "0.0-standin":
        raise RuntimeError("a numba module is already loaded: install the stand-in before importing the reference")
    m = types.ModuleType("numba")
    m.jit = m.njit = _identity
    m.vectorize = _vectorize
    m.guvectorize = guvectorize
    m.stencil = stencil
    m.__version__ = "0.0-standin"
    sys.modules["numba"] = m
    return m
