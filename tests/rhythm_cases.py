"""Shared by tests/test_rhythm_host.py and tests/test_rhythm_gpu.py: the golden fixture tests/golden/rhythm.npz and how its cases are called."""
import json
import os

import numpy as np

from rhythm_signals import SR, call_kwargs, make_inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rhythm.npz")
SIGNALS = ("y", "y0", "y0_f64", "y16", "silent", "pulses")


def load():
    z = np.load(GOLDEN)
    inputs = make_inputs()
    for k, v in inputs.items():  # the seeds rebuild the reference's inputs exactly
        assert float(z[f"sum_{k}"]) == float(np.sum(v, dtype=np.float64)), f"input {k} is not the one the fixture was made from"
    return z, json.loads(str(z["cases"])), inputs


def names(kind):
    z = np.load(GOLDEN)
    return [n for n, c in json.loads(str(z["cases"])).items() if c["fn"] == kind]


def from_signal(case):
    return case["input"] in SIGNALS


def sampled(z, name, res):
    """The columns of ``res`` the fixture stored for ``name``."""
    return res[..., z[f"cols_{name}"]] if f"cols_{name}" in z else res


def col_err(got, want):
    """max |got - want| per column over the column's max |want| (0 / 0 columns count as 0), the largest over all columns."""
    got, want = np.asarray(got), np.asarray(want)
    scale = np.max(np.abs(want), axis=-2, keepdims=True)
    err = np.max(np.abs(got - want), axis=-2, keepdims=True)
    return float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1), err))) if want.size else 0.0


__all__ = ["SR", "call_kwargs", "load", "names", "from_signal", "sampled", "col_err", "SIGNALS"]
