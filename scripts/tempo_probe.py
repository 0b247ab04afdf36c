"""Performance probe (GPU box): device-tensor tempo estimation on 256 x 30 s at 22 050 Hz.

    python scripts/tempo_probe.py            # onset_strength, tempo(y), tempogram(y), tempo(aggregate=None): CUDA-event medians, one JSON line
    python scripts/tempo_probe.py --once     # one call of each after a warm-up (for rocprofv3 --kernel-trace --stats)

tempo(y) is onset_strength's three launches plus the tempogram kernel in SUM mode and the finishing launch; tempogram(y) writes the
256 x 384 x 1292 float64 tempogram (1.016 GB)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import librosa_amd as L  # noqa: E402

SR = 22050


def median_ms(fn, iters, warmup=3):
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
    rng = np.random.default_rng(0)
    y = torch.from_numpy((0.1 * rng.standard_normal((256, 30 * SR))).astype(np.float32)).to("cuda")
    calls = dict(onset_strength=lambda: L.onset.onset_strength(y=y, sr=SR), tempo=lambda: L.feature.tempo(y=y, sr=SR),
                 tempogram=lambda: L.feature.tempogram(y=y, sr=SR), tempo_per_frame=lambda: L.feature.tempo(y=y, sr=SR, aggregate=None))
    if "--once" in sys.argv:
        for fn in calls.values():
            fn()
            torch.cuda.synchronize()
        for fn in calls.values():
            fn()
            torch.cuda.synchronize()
        return
    res = {}
    for name, fn in calls.items():
        med, mn = median_ms(fn, 20)
        res[f"{name}_ms"], res[f"{name}_min_ms"] = round(med, 4), round(mn, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
