"""Feature extraction: ``melspectrogram`` and ``mfcc`` on the hot path, and the rhythm features ``tempogram``, ``fourier_tempogram`` and
``tempo`` on the fused onset path (``librosa/feature/__init__.pyi:12-13``, ``librosa/feature/rhythm.py``)."""
from .rhythm import fourier_tempogram, tempo, tempogram
from .spectral import melspectrogram, mfcc

__all__ = ["melspectrogram", "mfcc", "tempogram", "fourier_tempogram", "tempo"]
