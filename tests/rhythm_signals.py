"""The inputs of tests/golden/rhythm.npz, rebuilt from seeds (scripts/make_rhythm_golden.py stores only their checksums)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import golden_cases  # noqa: E402

SR = 22050


def pulses(bpm, sr, seconds, seed):
    """A click train at ``bpm`` (decaying noise bursts) over a quiet noise floor: the reference's tests/test_beat.py builds its tempo
    fixtures the same way (clicks at a known tempo)."""
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    y = 0.01 * rng.standard_normal(n)
    step = 60.0 / bpm * sr
    burst = rng.standard_normal(int(0.02 * sr)) * np.exp(-np.arange(int(0.02 * sr)) / (0.004 * sr))
    for k in range(int(n / step)):
        i = int(round(k * step))
        m = min(len(burst), n - i)
        y[i : i + m] += burst[:m]
    return y.astype(np.float32)


def make_inputs():
    y = golden_cases.make_signal("mix", 6 * SR, 43, (2,), "float32")
    t = np.arange(6 * SR)
    y = (y * (1.0 + 3.0 * ((t % (SR // 2)) < 700))[None, :] * 0.25).astype(np.float32)  # bursts at 120 BPM
    rng = np.random.default_rng(11)
    inp = dict(y=y, y0=y[0], y16=pulses(100, 16000, 10, 5), silent=np.zeros(3 * SR, np.float32),
               pulses=np.stack([pulses(b, SR, 10, 20 + i) for i, b in enumerate((70, 96, 128, 150))]),
               env_rand=np.abs(rng.standard_normal((2, 2, 90))).astype(np.float32), env_short=np.abs(rng.standard_normal(50)).astype(np.float32),
               env_zero=np.zeros(60, np.float32), win_array=np.hamming(127))
    inp["y0_f64"] = inp["y0"].astype(np.float64)
    return inp


def call_kwargs(kw, inputs):
    """The stored call description -> keyword arguments of a real call (the tests use the same function through the JSON)."""
    import scipy.stats

    out = dict(kw)
    if out.get("window") == "ones":
        out["window"] = np.ones
    elif out.get("window") == "win_array":
        out["window"] = inputs["win_array"]
    if out.get("norm") == "inf":
        out["norm"] = np.inf
    if out.get("prior") == "uniform":
        out["prior"] = scipy.stats.uniform(30, 300)
    if "aggregate" in out:
        out["aggregate"] = {"none": None, "median": np.median}[out["aggregate"]]
    return out
