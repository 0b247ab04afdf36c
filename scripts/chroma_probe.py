"""Performance probe (GPU box): device-tensor chroma_stft on 256 x 30 s at 22 050 Hz, n_fft 2048, hop 512.

    python scripts/chroma_probe.py            # CUDA-event medians of 50 calls after a warm-up, one JSON line
    python scripts/chroma_probe.py --once     # one call of each after a warm-up (for rocprofv3 --kernel-trace --stats)

Timed: ``chroma_stft(y)`` end to end (the power launch, the chroma launch, the read-back of the non-finite flag); ``chroma_stft(S=S)`` on the
resident power spectrogram in the device layout (the frame-major kernel alone, plus that read-back) and on its C-contiguous copy (the
bin-major kernel); and ``_spectrogram(y, power=2)`` alone -- the unchanged power launch, the yardstick on the same box.  Rates: the
spectrogram's bytes (batch x frames x 1025 x 4) over the call's time, as read by the chroma kernels and as written by the power launch, next
to the 8 TB/s peak of the MI355X's HBM."""
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
    S = L._spectrogram(y=y, n_fft=N_FFT, hop_length=HOP, power=2)[0]
    Sc = S.contiguous()
    nbytes = S.numel() * 4
    kw = dict(sr=SR, tuning=0.0, n_fft=N_FFT, hop_length=HOP)
    calls = {
        "chroma_stft_y": lambda: L.feature.chroma_stft(y=y, **kw),
        "chroma_stft_y_unchecked": lambda: L.feature.chroma_stft(y=y, check_finite=False, **kw),
        "chroma_S_frame_major": lambda: L.feature.chroma_stft(S=S, sr=SR, tuning=0.0),
        "chroma_S_bin_major": lambda: L.feature.chroma_stft(S=Sc, sr=SR, tuning=0.0),
        "chroma_S_frame_major_c36": lambda: L.feature.chroma_stft(S=S, sr=SR, tuning=0.0, n_chroma=36),
        "power_spectrogram": lambda: L._spectrogram(y=y, n_fft=N_FFT, hop_length=HOP, power=2),
    }
    if "--once" in sys.argv:
        for _ in range(2):
            for fn in calls.values():
                fn()
                torch.cuda.synchronize()
        return
    res = {"batch": batch, "frames": int(S.shape[-1]), "spectrogram_bytes": nbytes}
    for name, fn in calls.items():
        med, mn = median_ms(fn, 50)
        res[f"{name}_ms"], res[f"{name}_min_ms"] = round(med, 4), round(mn, 4)
    for name in ("chroma_S_frame_major", "chroma_S_bin_major", "power_spectrogram"):
        rate = nbytes / (res[f"{name}_ms"] * 1e-3)
        res[f"{name}_TBps"], res[f"{name}_of_peak"] = round(rate / 1e12, 3), round(rate / PEAK_BYTES_PER_S, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
