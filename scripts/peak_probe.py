"""Performance probe (GPU box): device-tensor onset detection on 256 x 30 s, at 22 050 Hz / hop 512 and at 16 kHz / hop 160.

    python scripts/peak_probe.py            # onset_strength(y) and onset_detect(y, sparse=False) per method: CUDA-event medians of 100 calls, one JSON line
    python scripts/peak_probe.py --once     # one call of each after a warm-up (for rocprofv3 --kernel-trace --stats)
    python scripts/peak_probe.py --once --config 22k   # ... of one configuration only (22k | 16k)

onset_detect(y) is onset_strength's three launches (mean aggregate) and the picker's three (row statistics, candidates, selection);
onset_detect minus onset_strength is the picker stage, which includes the read-back of its two status flags (a stream synchronisation)."""
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
METHODS = ("greedy", "dp_count", "dp_value")


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
    """256 click trains of 30 s, tempi spread over 60-180 BPM: 16 distinct seeds tiled."""
    base = np.stack([pulses(60.0 + 120.0 * i / 15, sr, 30, 300 + i) for i in range(16)])
    return torch.from_numpy(np.tile(base, (16, 1))).to("cuda")


def main():
    res = {}
    only = sys.argv[sys.argv.index("--config") + 1] if "--config" in sys.argv else None
    for tag, sr, hop in CONFIGS:
        if only not in (None, tag):
            continue
        y = signals(sr)
        calls = {f"onset_strength_{tag}": lambda: L.onset.onset_strength(y=y, sr=sr, hop_length=hop)}
        for method in METHODS:
            calls[f"onset_detect_{method}_{tag}"] = lambda method=method: L.onset.onset_detect(y=y, sr=sr, hop_length=hop, sparse=False, method=method)
        calls[f"onset_detect_backtrack_row_{tag}"] = lambda: L.onset.onset_detect(y=y[0], sr=sr, hop_length=hop, backtrack=True)
        if "--once" in sys.argv:
            for _ in range(2):
                for fn in calls.values():
                    fn()
                    torch.cuda.synchronize()
            continue
        for name, fn in calls.items():
            med, mn = median_ms(fn, 100)
            res[f"{name}_ms"], res[f"{name}_min_ms"] = round(med, 4), round(mn, 4)
        for method in METHODS:
            res[f"picker_stage_{method}_{tag}_ms"] = round(res[f"onset_detect_{method}_{tag}_ms"] - res[f"onset_strength_{tag}_ms"], 4)
    if res:
        print(json.dumps(res))


if __name__ == "__main__":
    main()
