"""Performance probe (GPU box): device-tensor beat tracking on 256 x 30 s, at 22 050 Hz / hop 512 and at 16 kHz / hop 160.

    python scripts/beat_probe.py            # tempo(y), onset_strength(y, aggregate=np.median), beat_track(y, sparse=False): CUDA-event medians of 100 calls, one JSON line
    python scripts/beat_probe.py --once     # one call of each after a warm-up (for rocprofv3 --kernel-trace --stats)
    python scripts/beat_probe.py --once --config 22k   # ... of one configuration only (22k | 16k), so that a trace's per-kernel sums are its own

beat_track(y) is onset_strength's three launches (median aggregate), the tempogram kernel in SUM mode with its finishing launch, and the
tracker's three launches; beat_track minus tempo is the tracker stage (plus the median aggregate's extra cost over the mean)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import librosa_amd as L  # noqa: E402
from rhythm_signals import pulses  # noqa: E402

CONFIGS = (("22k", 22050, 512), ("16k", 16000, 160))


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


def signals(sr):
    """256 click trains of 30 s, tempi spread over 60-180 BPM: 16 distinct seeds tiled (the tracker's time does not depend on the noise draw)."""
    base = np.stack([pulses(60.0 + 120.0 * i / 15, sr, 30, 300 + i) for i in range(16)])
    return torch.from_numpy(np.tile(base, (16, 1))).to("cuda")


def main():
    res = {}
    only = sys.argv[sys.argv.index("--config") + 1] if "--config" in sys.argv else None
    for tag, sr, hop in CONFIGS:
        if only not in (None, tag):
            continue
        y = signals(sr)
        calls = {f"tempo_{tag}": lambda: L.feature.tempo(y=y, sr=sr, hop_length=hop),
                 f"onset_median_{tag}": lambda: L.onset.onset_strength(y=y, sr=sr, hop_length=hop, aggregate=np.median),
                 f"beat_track_{tag}": lambda: L.beat.beat_track(y=y, sr=sr, hop_length=hop, sparse=False)}
        if "--once" in sys.argv:
            for _ in range(2):
                for fn in calls.values():
                    fn()
                    torch.cuda.synchronize()
            continue
        for name, fn in calls.items():
            med, mn = median_ms(fn, 100)
            res[f"{name}_ms"], res[f"{name}_min_ms"] = round(med, 4), round(mn, 4)
        res[f"tracker_stage_{tag}_ms"] = round(res[f"beat_track_{tag}_ms"] - res[f"tempo_{tag}_ms"], 4)
    if res:
        print(json.dumps(res))


if __name__ == "__main__":
    main()
