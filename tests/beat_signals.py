"""The inputs and cases of tests/golden/beat.npz, rebuilt from seeds (scripts/make_beat_golden.py stores only the inputs' checksums)."""
import json
import os

import numpy as np

from rhythm_signals import SR, pulses
from rhythm_signals import make_inputs as _rhythm_inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beat.npz")

# the full-size batch: FULL_ROWS click trains of FULL_SECONDS with tempi spread evenly over 60-180 BPM; the reference's beats of FULL_STORED are in the fixture
FULL_ROWS, FULL_SECONDS = 256, 30
FULL_STORED = (0, 36, 73, 109, 146, 182, 219, 255)

# name -> (input, kwargs).  "y:<key>": the signal; "env:<key>" / "env64:<key>": the reference's onset_strength(aggregate=np.median) of that signal
# (as float64), given as onset_envelope; "raw:<key>": an envelope used as it is.  bpm "frames": the reference's tempo(aggregate=None) of the
# envelope (stored as bpm_<case>); prior "uniform": scipy.stats.uniform(60, 240).
_K16 = dict(sr=16000, hop_length=160)
CASES = {
    "y_mono": ("y:y0", dict()),
    "y_16k": ("y:y16", dict(_K16)),
    "y_f64": ("y:y0_f64", dict()),
    "y_hop441": ("y:y0", dict(hop_length=441)),
    "y_batch4": ("y:pulses", dict(sparse=False)),
    "env_f32": ("env:y0", dict()),
    "env_f64": ("env64:y0", dict()),
    "bpm_scalar": ("env:pulses", dict(bpm=100.0, sparse=False)),
    "bpm_channel": ("env:pulses", dict(bpm=[70.0, 96.0, 128.0, 150.0], sparse=False)),
    "bpm_frame": ("env:y16", dict(_K16, bpm="frames")),
    "tight_1e2": ("env:y16", dict(_K16, tightness=1e2)),
    "tight_1e4": ("env:y16", dict(_K16, tightness=1e4)),
    "tight_10": ("env:y16", dict(_K16, tightness=10)),
    "trim_false": ("env:y16", dict(_K16, trim=False)),
    "start_60": ("env:y0", dict(start_bpm=60)),
    "start_240": ("env:y0", dict(start_bpm=240)),
    "prior_uniform": ("env:y0", dict(prior="uniform")),
    "units_frames": ("env:y16", dict(_K16, units="frames")),
    "units_samples": ("env:y16", dict(_K16, units="samples")),
    "units_time": ("env:y16", dict(_K16, units="time")),
    "env_const": ("raw:env_const", dict()),
    "rand2": ("raw:env_rand2", dict(bpm=120.0)),
    "rand3": ("raw:env_rand3", dict(bpm=120.0)),
    "rand5": ("raw:env_rand5", dict(bpm=120.0)),
    "rand30": ("raw:env_rand30", dict(bpm=120.0)),
    # a window wider than the tracker's LDS ring: frames_per_beat = 1200, candidates up to 2400 frames back (the general loop, values from global scratch)
    "wide_window": ("raw:env_rand3000", dict(_K16, bpm=5.0)),
    "zero_sparse": ("raw:env_zero", dict()),
    "zero_dense": ("raw:env_zero2", dict(sparse=False)),
}


def full_bpm(i):
    return 60.0 + 120.0 * i / (FULL_ROWS - 1)


def full_signal(i):
    return pulses(full_bpm(i), SR, FULL_SECONDS, 1000 + i)


def make_inputs():
    r = _rhythm_inputs()
    rng = np.random.default_rng(77)
    inp = dict(y0=r["y0"], y0_f64=r["y0_f64"], y16=r["y16"], pulses=r["pulses"])
    for n in (2, 3, 5, 30):
        inp[f"env_rand{n}"] = np.abs(rng.standard_normal(n)).astype(np.float32)
    inp["env_rand3000"] = np.abs(np.random.default_rng(78).standard_normal(3000)).astype(np.float32)
    inp["env_const"] = np.ones(200, np.float32)
    inp["env_zero"] = np.zeros(100, np.float32)
    inp["env_zero2"] = np.zeros((2, 100), np.float32)
    return inp


def call_kwargs(kw, z=None, name=None):
    """The stored call description -> keyword arguments of a real call (``z``: the loaded fixture, for bpm="frames")."""
    import scipy.stats

    out = dict(kw)
    if out.get("prior") == "uniform":
        out["prior"] = scipy.stats.uniform(60, 240)
    if isinstance(out.get("bpm"), str):
        out["bpm"] = np.asarray(z[f"bpm_{name}"])
    elif isinstance(out.get("bpm"), list):
        out["bpm"] = np.asarray(out["bpm"], dtype=np.float64)
    return out


def load():
    z = np.load(GOLDEN)
    inputs = make_inputs()
    for k, v in inputs.items():  # the seeds rebuild the reference's inputs exactly
        assert float(z[f"sum_{k}"]) == float(np.sum(v, dtype=np.float64)), f"input {k} is not the one the fixture was made from"
    return z, json.loads(str(z["cases"])), inputs, json.loads(str(z["params"]))


def names():
    return list(CASES)
