"""Frequency-scale conversions feeding ``filters.mel`` (host-side float64 scalar math).

Same formulas, constants and argument meaning as ``librosa/core/convert.py`` (``hz_to_mel``
:1004-1058, ``mel_to_hz`` :1069-1121, ``fft_frequencies`` :1369-1391, ``mel_frequencies``
:1432-1511) so the resulting filterbank is bit-identical to the reference's.
"""
from __future__ import annotations

import numpy as np

# Slaney (Auditory Toolbox) mel scale: linear below 1 kHz, logarithmic above
_F_SP = 200.0 / 3
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = _MIN_LOG_HZ / _F_SP
_LOGSTEP = np.log(6.4) / 27.0


def hz_to_mel(frequencies, *, htk=False):
    f = np.asanyarray(frequencies)[()]
    if htk:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    mels = f / _F_SP
    if f.ndim:
        hi = f >= _MIN_LOG_HZ
        mels[hi] = _MIN_LOG_MEL + np.log(f[hi] / _MIN_LOG_HZ) / _LOGSTEP
    elif f >= _MIN_LOG_HZ:
        mels = _MIN_LOG_MEL + np.log(f / _MIN_LOG_HZ) / _LOGSTEP
    return mels


def mel_to_hz(mels, *, htk=False):
    m = np.asanyarray(mels)[()]
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    freqs = _F_SP * m
    if m.ndim:
        hi = m >= _MIN_LOG_MEL
        freqs[hi] = _MIN_LOG_HZ * np.exp(_LOGSTEP * (m[hi] - _MIN_LOG_MEL))
    elif m >= _MIN_LOG_MEL:
        freqs = _MIN_LOG_HZ * np.exp(_LOGSTEP * (m - _MIN_LOG_MEL))
    return freqs


def hz_to_octs(frequencies, *, tuning=0.0, bins_per_octave=12):
    """Frequencies (Hz) to fractional octave numbers relative to A0 / 2 = 27.5 Hz at ``tuning`` 0 (``librosa/core/convert.py:1146-1182``)."""
    A440 = 440.0 * 2.0 ** (tuning / bins_per_octave)
    octs = np.log2(np.asanyarray(frequencies) / (float(A440) / 16))
    return octs[()]


def octs_to_hz(octs, *, tuning=0.0, bins_per_octave=12):
    """Octave numbers to frequencies; the inverse of ``hz_to_octs`` (``librosa/core/convert.py:1204-1241``)."""
    A440 = 440.0 * 2.0 ** (tuning / bins_per_octave)
    return (float(A440) / 16) * (2.0 ** np.asanyarray(octs)[()])


def fft_frequencies(*, sr=22050, n_fft=2048):
    return np.fft.rfftfreq(n=n_fft, d=1.0 / sr)


def tempo_frequencies(n_bins, *, hop_length=512, sr=22050):
    """BPM of each lag of an autocorrelation tempogram; bin 0 is ``inf`` (``librosa/core/convert.py:1514-1544``)."""
    bin_frequencies = np.zeros(int(n_bins), dtype=np.float64)
    bin_frequencies[0] = np.inf
    bin_frequencies[1:] = 60.0 * sr / (hop_length * np.arange(1.0, n_bins))
    return bin_frequencies


def fourier_tempo_frequencies(*, sr=22050, win_length=384, hop_length=512):
    """BPM of each bin of a Fourier tempogram (``librosa/core/convert.py:1547-1579``)."""
    return fft_frequencies(sr=sr * 60 / float(hop_length), n_fft=win_length)


def frames_to_samples(frames, *, hop_length=512, n_fft=None):
    """Frame indices -> sample indices (``librosa/core/convert.py:88-129``)."""
    offset = 0
    if n_fft is not None:
        offset = int(n_fft // 2)
    return (np.asanyarray(frames) * hop_length + offset).astype(int)[()]


def samples_to_frames(samples, *, hop_length=512, n_fft=None):
    """Sample indices -> frame indices, ``floor((samples - n_fft // 2) / hop_length)`` (``librosa/core/convert.py:143-195``)."""
    offset = 0
    if n_fft is not None:
        offset = int(n_fft // 2)
    samples = np.asanyarray(samples)
    return np.asarray(np.floor((samples - offset) // hop_length), dtype=int)[()]


def frames_to_time(frames, *, sr=22050, hop_length=512, n_fft=None):
    """Frame indices -> seconds (``librosa/core/convert.py:214-256``)."""
    return samples_to_time(frames_to_samples(frames, hop_length=hop_length, n_fft=n_fft), sr=sr)


def time_to_frames(times, *, sr=22050, hop_length=512, n_fft=None):
    """Seconds -> frame indices (``librosa/core/convert.py:275-324``)."""
    return samples_to_frames(time_to_samples(times, sr=sr), hop_length=hop_length, n_fft=n_fft)


def time_to_samples(times, *, sr=22050):
    """Seconds -> sample indices, truncated (``librosa/core/convert.py:333-361``)."""
    return (np.asanyarray(times) * sr).astype(int)[()]


def samples_to_time(samples, *, sr=22050):
    """Sample indices -> seconds (``librosa/core/convert.py:370-405``)."""
    return np.asanyarray(samples)[()] / float(sr)


def mel_frequencies(n_mels=128, *, fmin=0.0, fmax=11025.0, htk=False):
    lo = hz_to_mel(fmin, htk=htk)
    hi = hz_to_mel(fmax, htk=htk)
    return mel_to_hz(np.linspace(lo, hi, n_mels), htk=htk)
