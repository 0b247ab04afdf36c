"""Feature extraction: ``melspectrogram`` and ``mfcc`` on the hot path, the chroma features ``chroma_stft`` and ``chroma_cqt`` behind the power
STFT and the constant-Q transform, and the rhythm features ``tempogram``, ``fourier_tempogram`` and ``tempo`` on the fused onset path
and the history embedding ``stack_memory``
(``librosa/feature/__init__.pyi:12-13``, ``librosa/feature/utils.py``, ``librosa/feature/spectral.py``, ``librosa/feature/rhythm.py``)."""
from .chroma import chroma_cqt, chroma_stft
from .rhythm import fourier_tempogram, tempo, tempogram
from .spectral import melspectrogram, mfcc
from .utils import stack_memory

__all__ = ["melspectrogram", "mfcc", "chroma_stft", "chroma_cqt", "tempogram", "fourier_tempogram", "tempo", "stack_memory"]
