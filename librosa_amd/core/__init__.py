"""Core spectral transforms on the hot path (``librosa/core/spectrum.py``, ``core/convert.py``)."""
from . import audio, convert, intervals, spectrum
from .audio import resample, stream
from .convert import (fft_frequencies, hz_to_octs, octs_to_hz, fourier_tempo_frequencies, frames_to_samples, frames_to_time, hz_to_mel, mel_frequencies, mel_to_hz, samples_to_frames, samples_to_time,
                      tempo_frequencies, time_to_frames, time_to_samples)
from .intervals import interval_frequencies
from .spectrum import _spectrogram, amplitude_to_db, db_to_amplitude, db_to_power, griffinlim, istft, magphase, pcen, phase_vocoder, power_to_db, stft
from . import constantq
from .constantq import cqt, vqt
from . import pitch
from .pitch import estimate_tuning, piptrack, pitch_tuning, pyin, yin

__all__ = ["audio", "constantq", "convert", "intervals", "pitch", "spectrum", "piptrack", "pitch_tuning", "estimate_tuning", "yin", "pyin", "hz_to_octs", "octs_to_hz", "cqt", "vqt", "interval_frequencies", "stream", "resample", "stft", "istft", "_spectrogram", "magphase", "griffinlim", "phase_vocoder", "pcen", "power_to_db", "amplitude_to_db", "db_to_power", "db_to_amplitude", "hz_to_mel", "mel_to_hz", "fft_frequencies", "tempo_frequencies", "fourier_tempo_frequencies", "mel_frequencies", "frames_to_samples", "samples_to_frames", "frames_to_time", "time_to_frames", "samples_to_time", "time_to_samples"]
