"""The one-wave n_fft = 2048 float32 cores on the exchange layouts of lra_fft.h (pass 0 -> 1 transposed, pass 1 -> last unpadded), through
the host simulator: the complex kernel body on radices 16-8-8 and 16-16-4 (variants 0 and 6), |X|^p, and the fused mel in its one-wave and
producer / consumer forms, at clips of 1, 2, 3, 5 and 12 frames with 1, 2 and 3 frames per slot.  No LDS race, no read of unwritten LDS (the
layouts' stores and reads cover the same units; the consumer's zero slot is written once, in its prologue), the two mel forms equal bit for
bit, and every result at the bars of tests/test_hostsim.py against the oracle.  librosa/core/spectrum.py:380-390, feature/spectral.py:2158-2160."""
import functools

import numpy as np
import pytest

import hostsim_util as H
import stft_oracle as O

SR, N_FFT = 22050, 2048
_CASES = [(nf, it, hop) for hop in (512, 256) for nf in (1, 2, 3, 5, 12) for it in (1, 2, 3)]


def _check_diag(d):
    assert d["races"] == 0 and d["uninit"] == 0, d


@functools.lru_cache(maxsize=None)
def _inputs(n_frames, hop):
    rng = np.random.default_rng(7000 + 10 * n_frames + hop)
    y = rng.standard_normal((2, (n_frames - 1) * hop + 37)).astype(np.float32)
    D = np.moveaxis(O.stft(y, n_fft=N_FFT, hop_length=hop), -1, -2)
    assert D.shape[1] == n_frames
    mel = {p: O.melspectrogram(y=y, sr=SR, n_fft=N_FFT, hop_length=hop, power=p, n_mels=128) for p in (1.0, 2.0)}
    for a in (y, D, *mel.values()):
        a.setflags(write=False)
    return y, D, mel


@pytest.mark.parametrize("n_frames,iters,hop", _CASES)
def test_complex_and_power(n_frames, iters, hop, monkeypatch):
    monkeypatch.delenv("LRA_SIM_PC", raising=False)
    y, Dref, _ = _inputs(n_frames, hop)
    win = O.get_window("hann", N_FFT)
    for variant, mult in ((0, 1), (6, 4)):  # (the 16-16-4 core's bars: test_stft_body_radix_16_16_4)
        D, d = H.stft(y, N_FFT, hop, win, mode=0, iters_per_wg=iters, variant=variant)
        assert d["v2"] == 1, d
        _check_diag(d)
        assert D.shape == Dref.shape and not np.isnan(D).any()
        assert np.abs(D - Dref).max() <= mult * 2e-6 * np.abs(Dref).max(), variant
        for power in (2.0, 1.0):
            S, d = H.stft(y, N_FFT, hop, win, mode=1, power=power, iters_per_wg=iters, variant=variant)
            assert d["v2"] == 1, d
            _check_diag(d)
            Sref = np.abs(Dref) ** power
            assert not np.isnan(S).any() and np.abs(S - Sref).max() <= (2 if variant else 1) * 4e-6 * Sref.max(), (variant, power)


@pytest.mark.parametrize("n_frames,iters,hop", _CASES)
@pytest.mark.parametrize("variant", [0, 6])
def test_mel_forms(n_frames, iters, hop, variant, monkeypatch):
    y, _, mel = _inputs(n_frames, hop)
    win = O.get_window("hann", N_FFT)
    B = O.mel(sr=SR, n_fft=N_FFT, n_mels=128)
    for power in (2.0, 1.0):
        Mref = mel[power]
        monkeypatch.delenv("LRA_SIM_PC", raising=False)
        M4, d4 = H.stft(y, N_FFT, hop, win, mode=4, power=power, mel_basis=B, iters_per_wg=iters, variant=variant)
        assert M4 is not None and d4["v2"] == 1, d4
        _check_diag(d4)
        assert M4.shape == Mref.shape and not np.isnan(M4).any()
        assert np.all(np.abs(M4 - Mref) <= 1e-5 * np.abs(Mref) + 1e-5 * Mref.max()), power
        monkeypatch.setenv("LRA_SIM_PC", "1")
        Mp, dp = H.stft(y, N_FFT, hop, win, mode=4, power=power, mel_basis=B, iters_per_wg=iters, variant=variant)
        if Mp is None:
            # the producer of |X| at hop n_fft / 4 does not fit three waves per SIMD on the 16-8-8 core (pc_fits_budget): the library keeps the one-wave form there
            assert (hop, power, variant) == (512, 1.0, 0), (dp, hop, power, variant)
            continue
        assert dp["v2"] == 2 and dp["NT"] == 192 and dp["lds"] <= 40 * 1024, dp
        _check_diag(dp)
        assert np.array_equal(Mp, M4), power
