"""Performance probe (GPU box): device-tensor yin on 256 x 30 s at 22 050 Hz, frame 2048, hop 512, 65 - 2093 Hz.

    python scripts/yin_probe.py            # CUDA-event medians of 10 calls after a warm-up, one JSON line
    python scripts/yin_probe.py --once     # one call of each after a warm-up (for rocprofv3 --kernel-trace --stats)

Timed: ``yin(y)`` end to end (the finite check of the samples, then one launch: samples in, one float64 per frame out), ``_yin_frames(y)``
(the dense CMND and shifts that pyin reads), and the complex ``stft`` of the same framing alone, the yardstick on the same box.  Per frame yin
runs two 1200-point complex float64 transforms (the real transform of 2400 points and its inverse) against the STFT's one 1024-point
complex float32 transform."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import librosa_amd as L  # noqa: E402
import stft_oracle as O  # noqa: E402
from librosa_amd.core import pitch as P  # noqa: E402

SR, FRAME, HOP, FMIN, FMAX = 22050, 2048, 512, 65.0, 2093.0


def median_ms(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def main():
    batch = int(sys.argv[sys.argv.index("--batch") + 1]) if "--batch" in sys.argv else 256
    y = torch.from_numpy(O.config_input(batch, n=30 * SR)).to("cuda")
    kw = dict(fmin=FMIN, fmax=FMAX, sr=SR, frame_length=FRAME, hop_length=HOP)
    calls = {
        "yin": lambda: L.yin(y, **kw),
        "yin_frames": lambda: P._yin_frames(y, **kw),
        "stft": lambda: L.stft(y, n_fft=FRAME, hop_length=HOP),
    }
    if "--once" in sys.argv:
        for _ in range(2):
            for fn in calls.values():
                fn()
                torch.cuda.synchronize()
        return
    f0 = L.yin(y, **kw)
    res = {"batch": batch, "frames": int(f0.shape[-1]), "f0_median_hz": float(f0.median())}
    for name, fn in calls.items():
        med, mn = median_ms(fn, 10)
        res[f"{name}_ms"], res[f"{name}_min_ms"] = round(med, 4), round(mn, 4)
    res["yin_over_stft"] = round(res["yin_ms"] / res["stft_ms"], 2)
    res["yin_us_per_frame"] = round(res["yin_ms"] * 1e3 / (batch * res["frames"]), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
