"""Performance probe (GPU box): device-tensor piptrack and estimate_tuning on 256 x 30 s at 22 050 Hz, n_fft 2048, hop 512.

    python scripts/tuning_probe.py            # CUDA-event medians of 30 calls after a warm-up, one JSON line
    python scripts/tuning_probe.py --once     # one call of each after a warm-up (for rocprofv3 --kernel-trace --stats)

Timed: the dense route ``piptrack(S=S)`` on the resident magnitude spectrogram in the device layout (one launch: S in, two arrays out) and on
its C-contiguous copy (the bin-major kernel); the fused route ``estimate_tuning(S=S)`` (the emitting launch, the radix select, the histogram,
the read-back of the counts row); ``estimate_tuning(y=y)`` end to end; and ``_spectrogram(y, power=1)`` alone, the yardstick on the same box.
Rates: the bytes each route has to move at least (dense: three times the spectrogram; fused: once) over the call's time, next to the 8 TB/s
peak of the MI355X's HBM."""
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

PEAK_BYTES_PER_S = 8.0e12
SR, N_FFT, HOP = 22050, 2048, 512


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
    batch = int(sys.argv[sys.argv.index("--batch") + 1]) if "--batch" in sys.argv else 256
    y = torch.from_numpy(O.config_input(batch, n=30 * SR)).to("cuda")
    S = L._spectrogram(y=y, n_fft=N_FFT, hop_length=HOP, power=1)[0]
    Sc = S.contiguous()
    nbytes = S.numel() * 4
    calls = {
        "piptrack_S_frame_major": (lambda: L.piptrack(S=S, sr=SR), 3),
        "piptrack_S_bin_major": (lambda: L.piptrack(S=Sc, sr=SR), 3),
        "estimate_tuning_S_frame_major": (lambda: L.estimate_tuning(S=S, sr=SR), 1),
        "estimate_tuning_S_bin_major": (lambda: L.estimate_tuning(S=Sc, sr=SR), 1),
        "estimate_tuning_y": (lambda: L.estimate_tuning(y=y, sr=SR, hop_length=HOP), 0),
        "magnitude_spectrogram": (lambda: L._spectrogram(y=y, n_fft=N_FFT, hop_length=HOP, power=1), 1),
    }
    if "--once" in sys.argv:
        for _ in range(2):
            for fn, _ in calls.values():
                fn()
                torch.cuda.synchronize()
        return
    res = {"batch": batch, "frames": int(S.shape[-1]), "spectrogram_bytes": nbytes, "tuning": L.estimate_tuning(S=S, sr=SR)}
    for name, (fn, passes) in calls.items():
        med, mn = median_ms(fn, 30)
        res[f"{name}_ms"], res[f"{name}_min_ms"] = round(med, 4), round(mn, 4)
        if passes:
            rate = passes * nbytes / (med * 1e-3)
            res[f"{name}_TBps"], res[f"{name}_of_peak"] = round(rate / 1e12, 3), round(rate / PEAK_BYTES_PER_S, 3)
    res["fused_over_dense"] = round(res["estimate_tuning_S_frame_major_ms"] / res["piptrack_S_frame_major_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
