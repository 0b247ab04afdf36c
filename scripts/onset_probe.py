"""Performance probe (GPU box): device-tensor onset_strength on 256 x 30 s at 22 050 Hz against melspectrogram alone on the same input.

    python scripts/onset_probe.py            # both timings, one JSON line
    python scripts/onset_probe.py --once     # one onset_strength call after a warm-up (for rocprofv3 --kernel-trace --stats)

The flux step reads the 256 x 128 x 1292 float32 mel (169 MB) once per lag term; the JSON line reports its cost as the difference of the
two medians and as the bandwidth that difference implies for one and for two reads of the mel."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import librosa_amd as L  # noqa: E402

SR = 22050


def median_ms(fn, iters, warmup=5):
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
    if "--once" in sys.argv:
        L.onset.onset_strength(y=y, sr=SR)
        torch.cuda.synchronize()
        L.onset.onset_strength(y=y, sr=SR)
        torch.cuda.synchronize()
        return
    mel_med, mel_min = median_ms(lambda: L.feature.melspectrogram(y=y, sr=SR, fmax=0.5 * SR), 30)
    ons_med, ons_min = median_ms(lambda: L.onset.onset_strength(y=y, sr=SR), 30)
    med_med, _ = median_ms(lambda: L.onset.onset_strength_multi(y=y, sr=SR, channels=[0, 32, 64, 96, 128], aggregate=np.median), 10)
    mel_bytes = 256 * 128 * 1292 * 4
    extra = ons_med - mel_med
    print(json.dumps(dict(mel_ms=round(mel_med, 4), mel_min_ms=round(mel_min, 4), onset_strength_ms=round(ons_med, 4), onset_min_ms=round(ons_min, 4),
                          onset_median_channels_ms=round(med_med, 4), flux_step_ms=round(extra, 4),
                          flux_gbps_one_read=round(mel_bytes / (extra * 1e-3) / 1e9, 1) if extra > 0 else None,
                          flux_gbps_two_reads=round(2 * mel_bytes / (extra * 1e-3) / 1e9, 1) if extra > 0 else None)))


if __name__ == "__main__":
    main()
