"""librosa_amd -- MI355X-native (gfx950) implementation of librosa's STFT -> mel-spectrogram hot
path and its inverse, behind librosa's own Python signatures.

    import librosa_amd as librosa
    D = librosa.stft(y, n_fft=2048, hop_length=512)
    M = librosa.feature.melspectrogram(y=y, sr=22050, n_fft=2048, hop_length=512, n_mels=128)
    y2 = librosa.istft(D, hop_length=512, length=len(y))

Only this path and the callers right next to it are provided -- ``magphase``, decibel scaling, ``feature.mfcc``, ``griffinlim``,
``phase_vocoder`` / ``effects.time_stretch``, ``decompose.hpss`` / ``effects.hpss``, ``pcen``, ``cqt`` / ``vqt``, ``stream``, ``resample``, ``onset.onset_strength`` / ``onset_strength_multi``,
``onset.onset_detect`` / ``onset_backtrack``, ``util.peak_pick``,
``feature.tempogram`` / ``fourier_tempogram`` / ``tempo``, ``beat.beat_track``, ``feature.chroma_stft`` / ``chroma_cqt`` (``tuning`` as a number), ``piptrack`` / ``pitch_tuning`` / ``estimate_tuning`` (which supplies that number on the device), ``yin``, ``pyin``,
``sequence.viterbi`` / ``viterbi_discriminative`` / ``viterbi_binary`` with the ``sequence.transition_*`` builders, ``sequence.dtw`` / ``dtw_backtracking``, ``sequence.rqa``, ``segment.cross_similarity`` / ``recurrence_matrix``,
``feature.stack_memory``, ``filters.diagonal_filter``, ``segment.path_enhance``, ``segment.recurrence_to_lag`` / ``lag_to_recurrence`` / ``timelag_filter``, ``util.shear``, and the frame / sample / time converters (see
DESIGN.md for the scope table).  Host-side Python validates
arguments exactly like the reference and builds the small float64 tables (window, mel basis, window
sum-square); all signal arithmetic runs in hand-written HIP kernels through the C ABI declared in
``include/librosa_amd.h``.  There is no CPU fallback: without the built library and a GPU, compute
calls raise ``librosa_amd.NativeError``.
"""
from . import beat, core, decompose, effects, feature, filters, onset, segment, sequence, util
from ._native import NativeError, device_count, get_context
from .core import (_spectrogram, amplitude_to_db, estimate_tuning, piptrack, pitch_tuning, yin, pyin, hz_to_octs, octs_to_hz, cqt, interval_frequencies, vqt, db_to_amplitude, db_to_power, fft_frequencies, fourier_tempo_frequencies, griffinlim, hz_to_mel, istft, magphase, pcen, phase_vocoder, mel_frequencies, mel_to_hz,
                   power_to_db, resample, stft, stream, tempo_frequencies, frames_to_samples, frames_to_time, samples_to_frames, samples_to_time, time_to_frames, time_to_samples)
from .util.exceptions import LibrosaError, ParameterError

__version__ = "0.1.0"

__all__ = ["beat", "core", "decompose", "effects", "feature", "filters", "onset", "segment", "sequence", "util", "stft", "istft", "_spectrogram", "magphase", "griffinlim", "phase_vocoder", "pcen", "cqt", "vqt", "interval_frequencies", "stream", "resample", "power_to_db", "amplitude_to_db", "db_to_power", "db_to_amplitude", "hz_to_mel", "mel_to_hz", "fft_frequencies", "tempo_frequencies", "fourier_tempo_frequencies", "mel_frequencies", "frames_to_samples", "samples_to_frames", "frames_to_time", "time_to_frames", "samples_to_time", "time_to_samples", "piptrack", "pitch_tuning", "estimate_tuning", "yin", "pyin", "hz_to_octs", "octs_to_hz",
           "LibrosaError", "ParameterError", "NativeError", "device_count", "get_context"]
