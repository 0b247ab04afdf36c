"""The n_fft = 2048 float32 kernels on the exchange layouts of lra_fft.h, on the device: complex and |X|^p (stft2_kernel on the 16-8-8 core
and, with ctx option variant = 6, on the 16-16-4 core) and the fused mel in its three forms (mel_pc 0: one wave per frame; 1: producer /
consumer on 16-8-8; 2: producer / consumer on 16-16-4), three clips of 1, 2, 3, 5, 12 and 1293 frames, hops n_fft / 4 and n_fft / 8, powers 2
and 1, through the public stft, _spectrogram and feature.melspectrogram.

Bars: complex and |X|^p as tests/test_gpu_parity.py (_stft_close; |d| <= 1e-4 |ref| + 1e-5 max|ref|); mel pure-relative 1e-4 against the oracle on
the noise-floored input; the producer / consumer forms within 2e-5 of the one-wave form; a batch equal to its clips run alone, bit for bit.
librosa/core/spectrum.py:380-390, :3000-3013, feature/spectral.py:2158-2160."""
import functools
import warnings

import numpy as np
import pytest

import geometry_cases as G
import stft_oracle as O

pytestmark = pytest.mark.gpu

warnings.filterwarnings("ignore", message="n_fft=.*is too large")

SR, N_FFT = 22050, 2048
_FRAMES = (1, 2, 3, 5, 12, 1293)


@functools.lru_cache(maxsize=None)
def _case(n_frames, hop):
    y = O.config_input(3, n=(n_frames - 1) * hop + 37)
    D = O.stft(y, n_fft=N_FFT, hop_length=hop)
    assert D.shape[-1] == n_frames
    for a in (y, D):
        a.setflags(write=False)
    return y, D


def _restore(ctx):
    for k, v in G.OPTION_DEFAULTS.items():
        ctx.set_option(k, v)


@pytest.mark.parametrize("hop", [512, 256])
@pytest.mark.parametrize("n_frames", _FRAMES)
def test_complex_and_power(n_frames, hop):
    import librosa_amd as L
    import torch

    ctx = L.get_context(0)
    y, Dref = _case(n_frames, hop)
    yt = torch.from_numpy(np.array(y)).to("cuda:0")
    scale = np.abs(Dref).max()
    try:
        for variant in (-1, 6):
            ctx.set_option("variant", variant)
            D = L.stft(yt, n_fft=N_FFT, hop_length=hop).cpu().numpy()
            assert D.shape == Dref.shape and D.dtype == Dref.dtype and not np.isnan(D).any()
            err = float(np.max(np.abs(D - Dref) - 1e-5 * np.abs(Dref)) / scale)
            print(f"variant {variant}: complex max (|d| - 1e-5 |ref|) / max|ref| {err:.3g}")
            assert np.all(np.abs(D - Dref) <= 1e-5 * np.abs(Dref) + 2e-6 * scale), (variant, err)
            for i in range(3):
                assert np.array_equal(L.stft(yt[i], n_fft=N_FFT, hop_length=hop).cpu().numpy(), D[i]), (variant, i)
            for power in (2.0, 1.0):
                Sref = np.abs(Dref) ** power
                S = L._spectrogram(y=yt, n_fft=N_FFT, hop_length=hop, power=power)[0].cpu().numpy()
                assert S.shape == Sref.shape and not np.isnan(S).any()
                perr = float(np.max(np.abs(S - Sref) - 1e-4 * np.abs(Sref)) / Sref.max())
                print(f"variant {variant} power {power}: max (|d| - 1e-4 |ref|) / max ref {perr:.3g}")
                assert np.all(np.abs(S - Sref) <= 1e-4 * np.abs(Sref) + 1e-5 * Sref.max()), (variant, power, perr)
                for i in range(3):
                    assert np.array_equal(L._spectrogram(y=yt[i], n_fft=N_FFT, hop_length=hop, power=power)[0].cpu().numpy(), S[i]), (variant, power, i)
    finally:
        _restore(ctx)


@pytest.mark.parametrize("hop,power", [(512, 2.0), (512, 1.0), (256, 2.0), (256, 1.0)])
@pytest.mark.parametrize("n_frames", _FRAMES)
def test_mel_forms(n_frames, hop, power):
    import librosa_amd as L
    import torch

    ctx = L.get_context(0)
    y, _ = _case(n_frames, hop)
    kw = dict(sr=SR, n_fft=N_FFT, hop_length=hop, n_mels=128, power=power)
    ref = O.melspectrogram(y=np.array(y), **kw)
    assert ref.shape[-1] == n_frames
    yt = torch.from_numpy(np.array(y)).to("cuda:0")
    try:
        outs = {}
        for pc in (0, 1, 2):
            ctx.set_option("mel_pc", pc)
            M = L.feature.melspectrogram(y=yt, **kw).cpu().numpy()
            assert M.shape == ref.shape and M.dtype == ref.dtype and not np.isnan(M).any()
            rel = float(np.max(np.abs(M - ref) / np.abs(ref)))
            print(f"mel_pc {pc}: max rel err against the oracle {rel:.3g}")
            assert np.all(np.abs(M - ref) <= 1e-4 * np.abs(ref)), (pc, rel)
            for i in range(3):
                assert np.array_equal(L.feature.melspectrogram(y=yt[i], **kw).cpu().numpy(), M[i]), (pc, i)
            outs[pc] = M
        for pc in (1, 2):
            both = float(np.max(np.abs(outs[pc] - outs[0]) / np.abs(outs[0])))
            print(f"mel_pc {pc} against 0: max rel diff {both:.3g}")
            assert np.all(np.abs(outs[pc] - outs[0]) <= 2e-5 * np.abs(outs[0])), (pc, both)
    finally:
        _restore(ctx)
