"""ctypes binding of ``include/librosa_amd.h`` (the gfx950 library ``_liblibrosa_amd.so``).

There is NO CPU fallback: if the shared library is missing or no HIP device is present, every
compute entry point raises :class:`NativeError` (a ``LibrosaError``).  The library is built
in-tree by ``__graft_entry__.build()`` / ``python -m librosa_amd.build``.
"""
from __future__ import annotations

import collections
import ctypes
import os
import threading
from ctypes import POINTER, byref, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p

import numpy as np

from .util.exceptions import LibrosaError, ParameterError

_HERE = os.path.dirname(os.path.abspath(__file__))
# LIBROSA_AMD_LIBRARY: load another build of the same ABI (kernel experiments, scripts/gpu_probe.py)
LIB_PATH = os.environ.get("LIBROSA_AMD_LIBRARY") or os.path.join(_HERE, "_liblibrosa_amd.so")

LRA_OK, LRA_EINVAL, LRA_EHIP, LRA_EROCFFT, LRA_ENODEV, LRA_ENOMEM = 0, -1, -2, -3, -4, -5
LRA_F32, LRA_F64 = 0, 1
PAD_MODES = {"constant": 0, "reflect": 1, "edge": 2, "symmetric": 3}


class NativeError(LibrosaError):
    """The HIP library is missing, or a HIP / rocFFT call failed."""


# name -> (restype, argtypes); every symbol declared in include/librosa_amd.h
SIGNATURES = {
    "lra_last_error": (c_char_p, []),
    "lra_version": (c_char_p, []),
    "lra_device_count": (c_int, [POINTER(c_int)]),
    "lra_ctx_create": (c_int, [c_int, POINTER(c_void_p)]),
    "lra_ctx_destroy": (None, [c_void_p]),
    "lra_ctx_set_stream": (c_int, [c_void_p, c_void_p]),
    "lra_ctx_side": (c_int, [c_void_p, c_int]),
    "lra_ctx_use_own_stream": (c_int, [c_void_p]),
    "lra_ctx_sync": (c_int, [c_void_p]),
    "lra_ctx_set_option": (c_int, [c_void_p, c_char_p, c_int]),
    "lra_ctx_device_name": (c_int, [c_void_p, c_char_p, c_size_t]),
    "lra_ctx_nonfinite_reset": (c_int, [c_void_p]),
    "lra_ctx_nonfinite_read": (c_int, [c_void_p, POINTER(c_int)]),
    "lra_stft_plan_is_fused": (c_int, [c_void_p]),
    "lra_stft_plan_tuned_variant": (c_int, [c_void_p, c_int]),
    "lra_istft_plan_tuned_variant": (c_int, [c_void_p]),
    "lra_malloc": (c_int, [c_void_p, c_size_t, POINTER(c_void_p)]),
    "lra_free": (c_int, [c_void_p, c_void_p]),
    "lra_malloc_placed": (c_int, [c_void_p, c_size_t, c_int, c_int64, c_int, POINTER(c_void_p), POINTER(c_float), POINTER(c_int)]),
    "lra_free_placed": (c_int, [c_void_p, c_void_p]),
    "lra_memset": (c_int, [c_void_p, c_void_p, c_int, c_size_t]),
    "lra_memcpy_h2d": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    "lra_memcpy_d2h": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    "lra_event_create": (c_int, [c_void_p, POINTER(c_void_p)]),
    "lra_event_destroy": (None, [c_void_p]),
    "lra_event_record": (c_int, [c_void_p]),
    "lra_event_elapsed_ms": (c_int, [c_void_p, c_void_p, POINTER(c_float)]),
    "lra_stft_plan_create": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, POINTER(c_void_p)]),
    "lra_stft_plan_destroy": (None, [c_void_p]),
    "lra_stft_num_frames": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "lra_stft_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p]),
    "lra_spectrogram_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_double, c_void_p]),
    "lra_mel_plan_create": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, POINTER(c_void_p)]),
    "lra_mel_plan_destroy": (None, [c_void_p]),
    "lra_melspectrogram_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_double, c_void_p]),
    "lra_mel_apply_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p]),
    "lra_istft_plan_create": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, POINTER(c_void_p)]),
    "lra_istft_plan_destroy": (None, [c_void_p]),
    "lra_istft_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64]),
    "lra_istft_exec_norm": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64]),
    "lra_transpose": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int]),
    "lra_probe_stream": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int64, c_int, c_int]),
    "lra_cqt_recursion_exec": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int, c_int, c_void_p, c_int64, c_int, c_int]),
    "lra_probe_stream_window": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int64, c_int, c_int]),
    "lra_pcg64_random_exec": (c_int, [c_void_p, POINTER(ctypes.c_uint64), ctypes.c_uint64, c_void_p, c_int64]),
    "lra_griffinlim_init_pcg64": (c_int, [c_void_p, POINTER(ctypes.c_uint64), c_void_p, c_void_p, c_int64, c_int, c_int64, c_int]),
    "lra_probe_stream_pitched": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int64, c_int, c_int, c_int64, c_int]),
    "lra_stft_exec_strided": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_int64, c_int64, c_double, c_void_p, c_int64]),
    "lra_item_absmax_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p]),
    "lra_item_max_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_void_p]),
    "lra_to_db_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_double, c_double, c_void_p, c_void_p, c_int, c_double]),
    "lra_from_db_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_double]),
    "lra_istft_exec_host": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64]),
    "lra_stft_exec_host": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int64, c_int64, c_double, c_void_p, c_int64, POINTER(c_int)]),
    "lra_comm_unique_id": (c_int, [c_void_p]),
    "lra_comm_init": (c_int, [c_void_p, c_int, c_int, c_void_p, POINTER(c_void_p)]),
    "lra_comm_allgather": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    "lra_comm_allgatherv": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_size_t), POINTER(c_size_t)]),
    "lra_comm_destroy": (None, [c_void_p]),
    "lra_phase_vocoder_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_int64, c_int]),
    "lra_griffinlim_init": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int]),
    "lra_griffinlim_update": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_double, c_double, c_int]),
    "lra_pcen_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_double, c_double, c_double, c_double, c_double, c_void_p, c_double, c_void_p]),
    "lra_maxfilter_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int64, c_int, c_int]),
    "lra_onset_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int64, c_int64, c_int,
                               c_double, c_double, c_void_p, c_int, c_void_p]),
    "lra_beat_work_bytes": (c_int64, [c_int64, c_int64, c_int]),
    "lra_beat_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_int, c_double, c_double, c_int, c_void_p, c_void_p, POINTER(c_int)]),
    "lra_peak_pick_work_bytes": (c_int64, [c_int64, c_int64, c_int]),
    "lra_peak_pick_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int64, c_int64, c_int64, c_int64, c_double, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                   POINTER(c_int)]),
    "lra_prev_minimum_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p]),
    "lra_tempogram_work_bytes": (c_int64, [c_int64, c_int64, c_int, c_int]),
    "lra_tempogram_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int)]),
    "lra_fir_decimate_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_int, c_int, c_double, c_double, c_int]),
    "lra_resample_poly_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_double, c_double, c_int]),
    "lra_resample_fft_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_double, c_int]),
    "lra_resample_band_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_double, c_double, c_double, c_int]),
    "lra_cqt_project_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int64, c_int, c_int, c_int, c_int, c_int]),
    "lra_cqt_octave_supported": (c_int, [c_int]),
    "lra_cqt_octave_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int]),
    "lra_magnitude_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int]),
    "lra_piptrack_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_int64, c_int64, c_int, c_double, c_void_p, c_double, c_double, c_int64,
                                  c_void_p, c_void_p, c_int64, c_int64, c_int64]),
    "lra_yin_lds_bytes": (c_int64, [c_int, c_int]),
    "lra_yin_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_double, c_double, c_int, c_void_p, c_void_p, c_void_p]),
    "lra_pyin_lds_bytes": (c_int64, [c_int, c_int]),
    "lra_pyin_obs_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_double, c_double, c_int, c_int, c_int, c_double,
                                  c_double, c_double, c_void_p, c_void_p]),
    "lra_pyin_finish_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int, c_double, c_void_p, c_void_p]),
    "lra_viterbi_lds_bytes": (c_int64, [c_int, c_int]),
    "lra_viterbi_prep_exec": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_int64, c_double, c_void_p, c_int, c_void_p, c_void_p, POINTER(c_int)]),
    "lra_viterbi_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p, c_int, c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lra_dtw_lds_bytes": (c_int64, [c_int, c_int, c_int]),
    "lra_dtw_cost_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, POINTER(c_int)]),
    "lra_dtw_prepare_exec": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p, POINTER(c_int)]),
    "lra_dtw_accumulate_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_int64, c_int, c_void_p, c_void_p]),
    "lra_dtw_widen_exec": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "lra_dtw_backtrack_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int64, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, POINTER(c_int64), POINTER(c_int)]),
    "lra_rqa_lds_bytes": (c_int64, [c_int, c_int]),
    "lra_rqa_score_exec": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_double, c_double, c_int, c_int, c_int, c_void_p, c_void_p]),
    "lra_rqa_argmax_exec": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p]),
    "lra_rqa_backtrack_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, POINTER(c_int64)]),
    "lra_knn_lds_bytes": (c_int64, [c_int, c_int, c_int]),
    "lra_knn_select_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int, c_int, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "lra_knn_mutual_exec": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "lra_knn_bandwidth_exec": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, POINTER(c_int), POINTER(c_int64)]),
    "lra_knn_bw_check_exec": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, POINTER(c_int)]),
    "lra_knn_emit_exec": (c_int, [c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, POINTER(c_int64)]),
    "lra_knn_dense_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int, c_int64, c_int, c_int, c_int, c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lra_enhance_lds_bytes": (c_int64, [c_int, c_int, c_int, c_int]),
    "lra_path_enhance_exec": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int, c_int, c_double, c_int, c_int, c_int, c_void_p, c_void_p]),
    "lra_shear_exec": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_void_p]),
    "lra_stack_memory_exec": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, ctypes.c_uint64, c_void_p]),
    "lra_tuning_work_bytes": (c_int64, [c_int64, c_int64, c_int64, c_int]),
    "lra_tuning_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_int64, c_int64, c_int, c_double, c_void_p, c_double, c_double, c_int64,
                                c_void_p, c_int64, c_double, c_void_p, c_void_p]),
    "lra_pitch_tuning_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_double, c_void_p]),
    "lra_chroma_exec": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_void_p, c_int64, c_int, c_double, c_int, c_void_p, c_void_p,
                        POINTER(c_int)]),
    "lra_magphase_exec": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_double, c_int]),
    "lra_hpss_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_double, c_double, c_double, c_int, c_int]),
    "lra_dct_exec": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int64, c_int, c_void_p, c_void_p, c_int, c_double, c_double, c_void_p, c_void_p, c_int, c_double]),
}

_lib = None
_lib_lock = threading.Lock()


def load_library():
    """dlopen the in-tree HIP library and attach signatures; raises NativeError when absent."""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise NativeError(
                    f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(librosa_amd has no CPU fallback)"
                )
            # PyTorch wheels bundle their own ROCm runtime (libamdhip64.so.7, libhsa-runtime64, librocfft
            # ... same SONAMEs as /opt/rocm).  Two different HIP runtimes in one process cannot both
            # own the device, so if torch is installed its runtime must be the one that is loaded first;
            # our library then binds to it through the shared SONAMEs.  Without torch the system ROCm
            # runtime is used.
            try:
                import torch  # noqa: F401
            except Exception:
                pass
            try:
                lib = ctypes.CDLL(LIB_PATH)
            except OSError as exc:  # missing libamdhip64 / librocfft
                raise NativeError(f"cannot load {LIB_PATH}: {exc}") from exc
            for name, (restype, argtypes) in SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = restype
                fn.argtypes = argtypes
            _lib = lib
    return _lib


def _check(rc):
    if rc == LRA_OK:
        return
    msg = load_library().lra_last_error().decode("utf-8", "replace")
    if rc == LRA_EINVAL:
        raise ParameterError(msg)
    raise NativeError(f"librosa_amd native error {rc}: {msg}")


def device_count():
    n = c_int(0)
    lib = load_library()
    rc = lib.lra_device_count(byref(n))
    return n.value if rc == LRA_OK else 0


def dtype_code(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return LRA_F32
    if dtype == np.float64:
        return LRA_F64
    raise ParameterError(f"unsupported real dtype {dtype}")


class DeviceBuffer:
    """Owning device allocation made through lra_malloc (NumPy path)."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = c_void_p()
        _check(ctx.lib.lra_malloc(ctx.handle, self.nbytes, byref(p)))
        self.ptr = p.value or 0

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        if arr.nbytes:
            _check(self.ctx.lib.lra_memcpy_h2d(self.ctx.handle, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        if out.nbytes:
            _check(self.ctx.lib.lra_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.ctx.lib.lra_free(self.ctx.handle, self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Event:
    def __init__(self, ctx):
        self.ctx = ctx
        h = c_void_p()
        _check(ctx.lib.lra_event_create(ctx.handle, byref(h)))
        self.handle = h

    def record(self):
        _check(self.ctx.lib.lra_event_record(self.handle))
        return self

    def elapsed_ms(self, stop):
        ms = c_float(0)
        _check(self.ctx.lib.lra_event_elapsed_ms(self.handle, stop.handle, byref(ms)))
        return ms.value

    def __del__(self):
        try:
            self.ctx.lib.lra_event_destroy(self.handle)
        except Exception:
            pass


class CqtOctave(ctypes.Structure):
    """``lra_cqt_octave`` (``include/librosa_amd.h``)."""
    _fields_ = [("n_fft", c_int), ("hop", c_int), ("bin0", c_int), ("row0", c_int), ("n_rows", c_int), ("halve", c_int), ("n", c_int64), ("row_ptr", c_void_p), ("col", c_void_p),
                ("val", c_void_p)]


class Context:
    """One device + stream + plan caches.  ``get_context(device)`` returns the shared instance."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = c_void_p()
        _check(self.lib.lra_ctx_create(int(device), byref(h)))
        self.handle = h
        self.device = int(device)
        # least-recently-used caches, bounded: a plan owns device tables (and, on the rocFFT path, scratch buffers)
        self._stft_plans = collections.OrderedDict()
        self._istft_plans = collections.OrderedDict()
        self._mel_plans = collections.OrderedDict()
        self._mel_by_id = {}
        self._tables = {}  # pool name -> OrderedDict (see device_table)
        self._lock = threading.RLock()
        self.call_lock = threading.RLock()  # held by _arrays.Session for the duration of one public call
        # placement-aware result buffers (lra_malloc_placed): `placement_retry` candidates per new buffer (0 = off; env LRA_PLACEMENT_RETRY), and the
        # buffers whose tensors have been dropped, kept for the next call of the same shape (their placement is already known to be a good one)
        # (default 4: on a box with the placement lottery the worst of five such buffers ran the complex STFT within 0.3 % of the best, 15 % between torch.empty ones;
        #  a box without it stops after two candidates, ~12 ms per new shape: profiles/r06b_bench_line.json)
        self.placement_retry = max(0, min(8, int(os.environ.get("LRA_PLACEMENT_RETRY", "4") or 0)))
        self._placed_free = {}   # (nbytes, row_bytes) -> [ptr]
        self._placed_log = []    # (nbytes, row_bytes, probe_ms, candidates tried) of every fresh allocation

    # -- context ------------------------------------------------------------------------------
    def device_name(self):
        buf = ctypes.create_string_buffer(256)
        _check(self.lib.lra_ctx_device_name(self.handle, buf, 256))
        return buf.value.decode()

    SIDE_FORK, SIDE_BACK, SIDE_JOIN, SIDE_END = 1, 2, 3, 4

    def side(self, mode):
        """A second stream of the context (``lra_ctx_side``): fork / back / join / end (= back if forked, then join)."""
        _check(self.lib.lra_ctx_side(self.handle, int(mode)))

    def set_stream(self, stream_ptr):
        """Enqueue on this hipStream_t (0 / None = HIP's default stream, torch's usual current stream)."""
        _check(self.lib.lra_ctx_set_stream(self.handle, c_void_p(stream_ptr or None)))

    def use_own_stream(self):
        _check(self.lib.lra_ctx_use_own_stream(self.handle))

    def sync(self):
        _check(self.lib.lra_ctx_sync(self.handle))

    def set_option(self, key, value):
        _check(self.lib.lra_ctx_set_option(self.handle, key.encode(), int(value)))
        if key == "placement_retry":
            self.placement_retry = max(0, min(8, int(value)))

    # -- placement-aware result buffers (include/librosa_amd.h, lra_malloc_placed) -----------------
    PLACED_MIN_BYTES = 256 << 20
    PLACED_KEEP_PER_SHAPE = 2
    PLACED_KEEP_BYTES = 12 << 30   # all recycled buffers together (variable-length inputs make a new shape per call: the oldest shapes go first)

    def placed_take(self, nbytes, row_bytes, rows_per_item=0):
        """Device pointer of a buffer of ``nbytes`` (rows of ``row_bytes``, ``rows_per_item`` of them per clip): a recycled one of that shape if there is
        one, else the best of ``placement_retry`` fresh candidates."""
        key = (int(nbytes), int(row_bytes), int(rows_per_item))
        with self._lock:
            free = self._placed_free.get(key)
            if free:
                return free.pop()
        p, ms, tried = c_void_p(), c_float(0), c_int(0)
        _check(self.lib.lra_malloc_placed(self.handle, key[0], key[1], key[2], int(self.placement_retry), byref(p), byref(ms), byref(tried)))
        with self._lock:
            self._placed_log.append((key[0], key[1], float(ms.value), int(tried.value)))
            del self._placed_log[:-64]
        return p.value

    def placed_give(self, nbytes, row_bytes, ptr, rows_per_item=0):
        """A placed buffer whose tensor is gone: kept for the next result of that shape, or released when enough are waiting."""
        key = (int(nbytes), int(row_bytes), int(rows_per_item))
        drop = []
        with self._lock:
            free = self._placed_free.pop(key, [])   # (re-inserted below: dict order = least recently returned shape first)
            if len(free) < self.PLACED_KEEP_PER_SHAPE and key[0] <= self.PLACED_KEEP_BYTES:
                free.append(ptr)
            else:
                drop.append(ptr)
            if free:
                self._placed_free[key] = free
            held = sum(k[0] * len(v) for k, v in self._placed_free.items())
            for k in list(self._placed_free):
                if held <= self.PLACED_KEEP_BYTES:
                    break
                if k == key and len(self._placed_free) > 1:
                    continue
                v = self._placed_free[k]
                while v and held > self.PLACED_KEEP_BYTES:
                    drop.append(v.pop(0))
                    held -= k[0]
                if not v:
                    del self._placed_free[k]
        for p in drop:
            try:
                self.lib.lra_free_placed(self.handle, c_void_p(p))
            except Exception:  # pragma: no cover - interpreter shutdown
                pass

    def placed_release_all(self):
        with self._lock:
            ptrs = [p for v in self._placed_free.values() for p in v]
            self._placed_free.clear()
        for p in ptrs:
            _check(self.lib.lra_free_placed(self.handle, c_void_p(p)))

    def nonfinite_reset(self):
        _check(self.lib.lra_ctx_nonfinite_reset(self.handle))

    def nonfinite_read(self):
        f = c_int(0)
        _check(self.lib.lra_ctx_nonfinite_read(self.handle, byref(f)))
        return bool(f.value)

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def event(self):
        return Event(self)

    PLAN_CACHE_SIZE = 48
    # device tables live in two LRU pools, each bounded by entries AND bytes: "small" (DCT bases, lifters, CQT bases, decimator taps: a few
    # KB each) and "large" (istft / griffinlim window sum-square envelopes: one float per output sample, a new key per (n_frames, length)).
    # Separate pools so that a stream of variable-length inverse transforms can neither pin gigabytes of HBM nor push the small tables out.
    TABLE_POOLS = {"small": (512, 64 << 20), "large": (8, 128 << 20)}

    def device_table(self, key, build, pool="small"):
        """Device pointer of a read-only table kept under ``key`` (LRU, bounded per pool by entry count and by bytes); ``build()`` returns the
        host array on a miss.  The upload is synchronous, so the table is usable from any stream of the device afterwards.  A table larger than
        a quarter of its pool's byte budget is not worth caching: callers check ``table_cacheable`` and upload per call instead."""
        max_entries, max_bytes = self.TABLE_POOLS[pool]
        with self._lock:
            tables = self._tables.setdefault(pool, collections.OrderedDict())
            buf = tables.get(key)
            if buf is not None:
                tables.move_to_end(key)
                return buf.ptr
            host = np.ascontiguousarray(build())
            buf = DeviceBuffer(self, max(host.nbytes, 16)).upload(host)
            tables[key] = buf
            while len(tables) > 1 and (len(tables) > max_entries or sum(b.nbytes for b in tables.values()) > max_bytes):
                _, old = tables.popitem(last=False)
                old.free()
            return buf.ptr

    def table_cacheable(self, nbytes, pool="small"):
        return int(nbytes) <= self.TABLE_POOLS[pool][1] // 4

    def table_bytes(self, pool=None):
        with self._lock:
            return sum(b.nbytes for name, t in self._tables.items() if pool in (None, name) for b in t.values())

    def _cached_plan(self, cache, key, create, destroy):
        """LRU lookup; on overflow the oldest plan is destroyed (hipFree synchronises with the device first)."""
        with self._lock:
            plan = cache.get(key)
            if plan is not None:
                cache.move_to_end(key)
                return plan
            plan = create()
            cache[key] = plan
            while len(cache) > self.PLAN_CACHE_SIZE:
                _, old = cache.popitem(last=False)
                destroy(old)
            return plan

    # -- plans (cached; keyed by the bytes of the host tables so any window spec works) -----------
    def stft_plan(self, n_fft, hop, window, center, pad_mode, dtype):
        window = np.ascontiguousarray(window, dtype=dtype)
        key = (int(n_fft), int(hop), window.tobytes(), bool(center), pad_mode, np.dtype(dtype).str)

        def create():
            h = c_void_p()
            _check(self.lib.lra_stft_plan_create(self.handle, int(n_fft), int(hop), window.ctypes.data, int(bool(center)), PAD_MODES[pad_mode], dtype_code(dtype), byref(h)))
            return h

        return self._cached_plan(self._stft_plans, key, create, self.lib.lra_stft_plan_destroy)

    def istft_plan(self, n_fft, hop, window, center, dtype):
        window = np.ascontiguousarray(window, dtype=dtype)
        key = (int(n_fft), int(hop), window.tobytes(), bool(center), np.dtype(dtype).str)

        def create():
            h = c_void_p()
            _check(self.lib.lra_istft_plan_create(self.handle, int(n_fft), int(hop), window.ctypes.data, int(bool(center)), dtype_code(dtype), byref(h)))
            return h

        return self._cached_plan(self._istft_plans, key, create, self.lib.lra_istft_plan_destroy)

    def mel_plan(self, basis):
        # Read-only arrays (what filters.mel_cached hands out) are recognised by identity: hashing the 525 KB of a 128 x 1025
        # basis on every call cost more host time than the kernel it configures takes to run.
        fast = isinstance(basis, np.ndarray) and not basis.flags.writeable and basis.flags.c_contiguous
        if fast:
            hit = self._mel_by_id.get(id(basis))
            if hit is not None and hit[0] is basis:
                plan = self._mel_plans.get(hit[1])
                if plan is not None:
                    return plan
        basis = np.ascontiguousarray(basis)
        key = (basis.shape, basis.dtype.str, basis.tobytes())
        if fast:
            if len(self._mel_by_id) > 4 * self.PLAN_CACHE_SIZE:
                self._mel_by_id.clear()
            self._mel_by_id[id(basis)] = (basis, key)

        def create():
            h = c_void_p()
            _check(self.lib.lra_mel_plan_create(self.handle, int(basis.shape[0]), int(basis.shape[1]), basis.ctypes.data, dtype_code(basis.dtype), byref(h)))
            return h

        return self._cached_plan(self._mel_plans, key, create, self.lib.lra_mel_plan_destroy)

    # -- execution ----------------------------------------------------------------------------------
    def stft_num_frames(self, plan, n):
        out = c_int64(0)
        _check(self.lib.lra_stft_num_frames(plan, int(n), byref(out)))
        return out.value

    def stft_is_fused(self, plan):
        return bool(self.lib.lra_stft_plan_is_fused(plan))

    def tuned_variant(self, plan, mode=None):
        """Kernel variant an stft plan (mode 0/1/2) or istft plan (mode None) settled on; -1 = not measured."""
        if mode is None:
            return int(self.lib.lra_istft_plan_tuned_variant(plan))
        return int(self.lib.lra_stft_plan_tuned_variant(plan, int(mode)))

    def stft_exec(self, plan, y_ptr, batch, n, y_stride, out_ptr):
        _check(self.lib.lra_stft_exec(plan, c_void_p(y_ptr), batch, n, y_stride, c_void_p(out_ptr)))

    def spectrogram_exec(self, plan, y_ptr, batch, n, y_stride, power, out_ptr):
        _check(self.lib.lra_spectrogram_exec(plan, c_void_p(y_ptr), batch, n, y_stride, float(power), c_void_p(out_ptr)))

    def stft_exec_strided(self, plan, kind, y_ptr, batch, n, y_stride, power, out_ptr, out_frame_stride):
        """kind 0 = complex spectrum, 1 = ``|X|**power``, rows ``out_frame_stride`` elements apart (fused power-of-two plans; ``include/librosa_amd.h``)."""
        _check(self.lib.lra_stft_exec_strided(plan, int(kind), c_void_p(y_ptr), batch, n, y_stride, float(power), c_void_p(out_ptr), int(out_frame_stride)))

    def melspectrogram_exec(self, plan, mel_plan, y_ptr, batch, n, y_stride, power, out_ptr):
        _check(self.lib.lra_melspectrogram_exec(plan, mel_plan, c_void_p(y_ptr), batch, n, y_stride, float(power), c_void_p(out_ptr)))

    def stft_exec_host(self, plan, mel_plan, kind, y_host_ptr, batch, n, y_stride, power, out_host_ptr, out_item_stride=0):
        """Host buffers in, host buffers out (chunked, overlapped staging); returns the non-finite flag."""
        flag = c_int(0)
        _check(self.lib.lra_stft_exec_host(plan, mel_plan, int(kind), c_void_p(y_host_ptr), batch, n, y_stride, float(power), c_void_p(out_host_ptr), int(out_item_stride), ctypes.byref(flag)))
        return bool(flag.value)

    def istft_exec_host(self, plan, d_host_ptr, batch, n_frames, n_used, wss_host_ptr, y_host_ptr, out_len, y_stride):
        _check(self.lib.lra_istft_exec_host(plan, c_void_p(d_host_ptr), batch, n_frames, n_used, c_void_p(wss_host_ptr), c_void_p(y_host_ptr), out_len, y_stride))

    def mel_apply_exec(self, mel_plan, s_ptr, batch, n_frames, batch_stride, bin_stride, frame_stride, out_ptr):
        _check(self.lib.lra_mel_apply_exec(mel_plan, c_void_p(s_ptr), batch, n_frames, batch_stride, bin_stride, frame_stride, c_void_p(out_ptr)))

    def istft_exec_norm(self, plan, d_ptr, batch, d_batch_stride, d_frame_stride, n_used, norm_ptr, y_ptr, out_len, y_stride):
        """``istft_exec`` with the normalisation given as factors (``1 / wss`` where ``wss > tiny``, else 1; ``spectrum.wss_to_norm``)."""
        _check(self.lib.lra_istft_exec_norm(plan, c_void_p(d_ptr), batch, d_batch_stride, d_frame_stride, n_used, c_void_p(norm_ptr), c_void_p(y_ptr), out_len, y_stride))

    def istft_exec(self, plan, d_ptr, batch, d_batch_stride, d_frame_stride, n_used, wss_ptr, y_ptr, out_len, y_stride):
        _check(self.lib.lra_istft_exec(plan, c_void_p(d_ptr), batch, d_batch_stride, d_frame_stride, n_used, c_void_p(wss_ptr), c_void_p(y_ptr), out_len, y_stride))

    def item_absmax_exec(self, x_ptr, batch, per_item, dtype, out_ptr):
        _check(self.lib.lra_item_absmax_exec(self.handle, c_void_p(x_ptr), batch, per_item, dtype_code(dtype), c_void_p(out_ptr)))

    def item_max_exec(self, x_ptr, batch, per_item, dtype, out_ptr, absolute):
        """Per-item maximum of |x| (``absolute``: amplitude_to_db) or of max(x, 0) (power_to_db on real input, which stays signed)."""
        _check(self.lib.lra_item_max_exec(self.handle, c_void_p(x_ptr), batch, per_item, dtype_code(dtype), int(bool(absolute)), c_void_p(out_ptr)))

    def to_db_exec(self, x_ptr, out_ptr, batch, per_item, dtype, amplitude, amin, ref_scalar, ref_items_ptr, item_max_ptr, top_db):
        _check(self.lib.lra_to_db_exec(self.handle, c_void_p(x_ptr), c_void_p(out_ptr), batch, per_item, dtype_code(dtype), int(bool(amplitude)), float(amin), float(ref_scalar),
                                       c_void_p(ref_items_ptr or None), c_void_p(item_max_ptr or None), int(top_db is not None), float(top_db if top_db is not None else 0.0)))

    def from_db_exec(self, x_ptr, out_ptr, count, dtype, amplitude, ref):
        _check(self.lib.lra_from_db_exec(self.handle, c_void_p(x_ptr), c_void_p(out_ptr), count, dtype_code(dtype), int(bool(amplitude)), float(ref)))

    def dct_exec(self, s_ptr, out_ptr, batch, n_in, n_out, n_frames, dtype, basis_ptr, lift_ptr, fuse_db=False, amin=1e-10, ref_scalar=1.0, ref_items_ptr=None, item_max_ptr=None, top_db=None):
        _check(self.lib.lra_dct_exec(self.handle, c_void_p(s_ptr), c_void_p(out_ptr), batch, n_in, n_out, n_frames, dtype_code(dtype), c_void_p(basis_ptr), c_void_p(lift_ptr),
                                     int(bool(fuse_db)), float(amin), float(ref_scalar), c_void_p(ref_items_ptr or None), c_void_p(item_max_ptr or None), int(top_db is not None),
                                     float(top_db if top_db is not None else 0.0)))

    def phase_vocoder_exec(self, d_ptr, out_ptr, batch, n_frames, n_bins, t_out, dtype):
        t = np.ascontiguousarray(t_out, dtype=np.float64)
        _check(self.lib.lra_phase_vocoder_exec(self.handle, c_void_p(d_ptr), c_void_p(out_ptr), batch, n_frames, n_bins, c_void_p(t.ctypes.data), len(t), dtype_code(dtype)))

    def pcen_exec(self, s_ptr, ref_ptr, out_ptr, rows, n_frames, dtype, b, gain, bias, power, eps, zi_ptr, zi_scalar, zf_ptr):
        _check(self.lib.lra_pcen_exec(self.handle, c_void_p(s_ptr), c_void_p(ref_ptr or None), c_void_p(out_ptr), rows, n_frames, dtype_code(dtype), float(b), float(gain), float(bias),
                                      float(power), float(eps), c_void_p(zi_ptr or None), float(zi_scalar), c_void_p(zf_ptr or None)))

    def maxfilter_exec(self, s_ptr, out_ptr, outer, n_bands, inner, size, dtype):
        _check(self.lib.lra_maxfilter_exec(self.handle, c_void_p(s_ptr), c_void_p(out_ptr), outer, n_bands, inner, int(size), dtype_code(dtype)))

    def onset_exec(self, s_ptr, ref_ptr, out_ptr, batch, n_bands, n_frames, dtype, lag, max_size, aggregate, ch_off_ptr, ch_band_ptr, n_ch, max_ch_bands, pad, n_out,
                   item_max_ptr=None, amin=1e-10, top_db=80.0, detrend_env_ptr=None):
        """Spectral-flux onset envelope (``include/librosa_amd.h``: lra_onset_exec).  ``item_max_ptr`` given: ``S`` is a power spectrogram whose
        decibels (``power_to_db(|S|, amin=amin, top_db=top_db)``) are taken on the fly; ``detrend_env_ptr`` given: the rows are detrended into
        a float64 ``out`` through that scratch."""
        _check(self.lib.lra_onset_exec(self.handle, c_void_p(s_ptr), c_void_p(ref_ptr or None), c_void_p(out_ptr), int(batch), int(n_bands), int(n_frames), dtype_code(dtype), int(lag),
                                       int(max_size), int(aggregate), c_void_p(ch_off_ptr or None), c_void_p(ch_band_ptr or None), int(n_ch), int(max_ch_bands), int(pad), int(n_out),
                                       int(item_max_ptr is not None), float(amin), float(top_db), c_void_p(item_max_ptr or None), int(detrend_env_ptr is not None),
                                       c_void_p(detrend_env_ptr or None)))

    def tempogram_work_bytes(self, batch, n_frames, win_length, mode):
        return int(self.lib.lra_tempogram_work_bytes(int(batch), int(n_frames), int(win_length), int(mode)))

    def tempogram_exec(self, env_ptr, batch, n, dtype, win_length, center, window_ptr, norm, mode, logprior_ptr, bpms_ptr, out_ptr, work_ptr):
        """Autocorrelation tempogram / tempo of [batch][n] envelopes (``include/librosa_amd.h``: lra_tempogram_exec).  Returns True when a
        column of the autocorrelation is not finite (this waits for the stream)."""
        flag = c_int(0)
        _check(self.lib.lra_tempogram_exec(self.handle, c_void_p(env_ptr), int(batch), int(n), dtype_code(dtype), int(win_length), int(bool(center)), c_void_p(window_ptr), int(norm),
                                           int(mode), c_void_p(logprior_ptr or None), c_void_p(bpms_ptr or None), c_void_p(out_ptr), c_void_p(work_ptr), byref(flag)))
        return bool(flag.value)

    def beat_work_bytes(self, batch, n, bpm_mode):
        return int(self.lib.lra_beat_work_bytes(int(batch), int(n), int(bpm_mode)))

    def beat_exec(self, env_ptr, batch, n, dtype, bpm_ptr, bpm_mode, frame_rate, tightness, trim, out_ptr, work_ptr):
        """The beat tracker on [batch][n] envelopes (``include/librosa_amd.h``: lra_beat_exec).  Returns True when some entry of the envelopes
        is non-zero (this waits for the stream)."""
        flag = c_int(0)
        _check(self.lib.lra_beat_exec(self.handle, c_void_p(env_ptr), int(batch), int(n), dtype_code(dtype), c_void_p(bpm_ptr), int(bpm_mode), float(frame_rate), float(tightness),
                                      int(bool(trim)), c_void_p(out_ptr), c_void_p(work_ptr), byref(flag)))
        return bool(flag.value)

    def peak_pick_work_bytes(self, batch, n, method):
        return int(self.lib.lra_peak_pick_work_bytes(int(batch), int(n), int(method)))

    def peak_pick_exec(self, x_ptr, batch, n, dtype, normalize, pre_max, post_max, pre_avg, post_avg, delta, wait, method, out_ptr, norm_ptr, work_ptr, status=True):
        """The peak picker on [batch][n] rows (``include/librosa_amd.h``: lra_peak_pick_exec).  Returns (some entry non-zero, every entry finite)
        of the normalised rows (this waits for the stream), or (None, None) with ``status=False`` (nothing is read back)."""
        flag = c_int(0)
        big = 2**62  # (a window or a dead time beyond the row counts as the row's length)
        _check(self.lib.lra_peak_pick_exec(self.handle, c_void_p(x_ptr), int(batch), int(n), dtype_code(dtype), int(bool(normalize)), min(int(pre_max), big), min(int(post_max), big),
                                           min(int(pre_avg), big), min(int(post_avg), big), float(delta), min(int(wait), big), int(method), c_void_p(out_ptr),
                                           c_void_p(norm_ptr or None), c_void_p(work_ptr), byref(flag) if status else None))
        return (bool(flag.value & 1), bool(flag.value & 2)) if status else (None, None)

    def prev_minimum_exec(self, energy_ptr, batch, m, dtype, out_ptr):
        """The preceding-minimum rows of [batch][m] energy rows (lra_prev_minimum_exec)."""
        _check(self.lib.lra_prev_minimum_exec(self.handle, c_void_p(energy_ptr), int(batch), int(m), dtype_code(dtype), c_void_p(out_ptr)))

    def fir_decimate_exec(self, x_ptr, out_ptr, batch, n_in, n_out, taps_ptr, n_taps, down, first, div, mul, dtype):
        _check(self.lib.lra_fir_decimate_exec(self.handle, c_void_p(x_ptr), c_void_p(out_ptr), batch, n_in, n_out, c_void_p(taps_ptr), int(n_taps), int(down), int(first), float(div),
                                              float(mul), dtype_code(dtype)))

    def resample_poly_exec(self, x_ptr, out_ptr, batch, n_in, n_out, taps_ptr, n_taps, up, down, first, div, mul, dtype):
        _check(self.lib.lra_resample_poly_exec(self.handle, c_void_p(x_ptr), c_void_p(out_ptr), batch, n_in, n_out, c_void_p(taps_ptr), int(n_taps), int(up), int(down), int(first),
                                               float(div), float(mul), dtype_code(dtype)))

    def resample_fft_exec(self, x_ptr, out_ptr, batch, n_in, n_out, gain, dtype):
        _check(self.lib.lra_resample_fft_exec(self.handle, c_void_p(x_ptr), c_void_p(out_ptr), batch, n_in, n_out, float(gain), dtype_code(dtype)))

    def resample_band_exec(self, x_ptr, out_ptr, batch, n_in, n_out, fft_in, fft_out, k_mid, k_sigma, gain, dtype):
        _check(self.lib.lra_resample_band_exec(self.handle, c_void_p(x_ptr), c_void_p(out_ptr), batch, n_in, n_out, int(fft_in), int(fft_out), float(k_mid), float(k_sigma), float(gain),
                                               dtype_code(dtype)))

    def cqt_project_exec(self, d_ptr, out_ptr, row_ptr, col_ptr, val_ptr, sqrt_len_ptr, batch, frames_in, n_bins, n_frames, n_total, bin0, row0, n_rows, dtype):
        _check(self.lib.lra_cqt_project_exec(self.handle, c_void_p(d_ptr), c_void_p(out_ptr), c_void_p(row_ptr), c_void_p(col_ptr), c_void_p(val_ptr), c_void_p(sqrt_len_ptr or None), batch,
                                             frames_in, int(n_bins), n_frames, int(n_total), int(bin0), int(row0), int(n_rows), dtype_code(dtype)))

    def cqt_octave_supported(self, n_fft):
        return bool(self.lib.lra_cqt_octave_supported(int(n_fft)))

    def cqt_octave_exec(self, y_ptr, batch, n, y_stride, n_fft, hop, pad_mode, row_ptr, col_ptr, val_ptr, sqrt_len_ptr, out_ptr, n_frames, n_total, bin0, row0, n_rows, dtype):
        """One constant-Q octave in one launch (``include/librosa_amd.h``): STFT with a rectangular window + sparse projection + scaling + stacking."""
        _check(self.lib.lra_cqt_octave_exec(self.handle, c_void_p(y_ptr), batch, n, y_stride, n_fft, hop, PAD_MODES[pad_mode], c_void_p(row_ptr), c_void_p(col_ptr), c_void_p(val_ptr),
                                            c_void_p(sqrt_len_ptr) if sqrt_len_ptr else None, c_void_p(out_ptr), n_frames, n_total, bin0, row0, n_rows, dtype_code(dtype)))

    def cqt_recursion_exec(self, y_ptr, batch, octaves, pad_mode, sqrt_len_ptr, out_ptr, n_frames, n_total, taps_ptr, n_taps, first, scratch_ptr, scratch_bytes, overlap, dtype):
        """The octave recursion of one cqt / vqt call in one native call; ``octaves``: a ``CqtOctave`` ctypes array (``include/librosa_amd.h``: lra_cqt_octave)."""
        _check(self.lib.lra_cqt_recursion_exec(self.handle, c_void_p(y_ptr), batch, ctypes.cast(octaves, c_void_p), len(octaves), PAD_MODES[pad_mode], c_void_p(sqrt_len_ptr) if sqrt_len_ptr else None,
                                               c_void_p(out_ptr), n_frames, int(n_total), c_void_p(taps_ptr) if taps_ptr else None, int(n_taps), int(first), c_void_p(scratch_ptr) if scratch_ptr else None,
                                               int(scratch_bytes), int(bool(overlap)), dtype_code(dtype)))

    CHROMA_NORMS = {None: 0, 1: 1, 2: 2, float("inf"): 3}   # the LRA_CHROMA_NORM_* values

    def chroma_exec(self, x_ptr, batch, n_bins, n_frames, batch_stride, bin_stride, frame_stride, dtype, w_ptr, n_chroma, norm_code, threshold, out_ptr, work_ptr):
        """Chroma projection + threshold + per-frame normalisation (``include/librosa_amd.h``: lra_chroma_exec); ``threshold=None`` skips the
        threshold.  Returns True when some raw value is not finite (this waits for the stream)."""
        flag = c_int(0)
        _check(self.lib.lra_chroma_exec(self.handle, c_void_p(x_ptr), int(batch), int(n_bins), int(n_frames), int(batch_stride), int(bin_stride), int(frame_stride), dtype_code(dtype),
                                        c_void_p(w_ptr), int(n_chroma), int(norm_code), 0.0 if threshold is None else float(threshold), int(threshold is not None), c_void_p(out_ptr),
                                        c_void_p(work_ptr), byref(flag)))
        return bool(flag.value)

    YIN_F0, YIN_FRAMES = 0, 1   # the LRA_YIN_* values

    def yin_exec(self, y_ptr, batch, n, dtype, frame_length, hop_length, center, pad_mode, min_period, max_period, trough_threshold, sr, mode, f0_ptr=0, frames_ptr=0, shifts_ptr=0):
        """YIN's f0 per frame, or the CMND and the parabolic shifts of every lag (``include/librosa_amd.h``: lra_yin_exec); ``pad_mode``: np.pad's name."""
        _check(self.lib.lra_yin_exec(self.handle, c_void_p(y_ptr), int(batch), int(n), dtype_code(dtype), int(frame_length), int(hop_length), int(bool(center)),
                                     {"constant": 0, "reflect": 1, "edge": 2, "symmetric": 3}[pad_mode], int(min_period), int(max_period), float(trough_threshold), float(sr), int(mode),
                                     c_void_p(f0_ptr or None), c_void_p(frames_ptr or None), c_void_p(shifts_ptr or None)))

    def pyin_obs_exec(self, cmnd_ptr, shifts_ptr, clips, n_lags, n_frames, thresholds_ptr, beta_ptr, beta_prefix_ptr, boltz_e_ptr, boltz_fact_ptr, n_thresholds, sr, fmin, min_period,
                      n_pitch_bins, n_bins_per_semitone, no_trough_prob, tiny, log_tiny, log_prob_ptr, voiced_prob_ptr):
        """pYIN's log observation table [clip][frame][state] and voiced_prob from the CMND and the shifts (``include/librosa_amd.h``: lra_pyin_obs_exec)."""
        _check(self.lib.lra_pyin_obs_exec(self.handle, c_void_p(cmnd_ptr), c_void_p(shifts_ptr), int(clips), int(n_lags), int(n_frames), c_void_p(thresholds_ptr), c_void_p(beta_ptr),
                                          c_void_p(beta_prefix_ptr), c_void_p(boltz_e_ptr), c_void_p(boltz_fact_ptr), int(n_thresholds), float(sr), float(fmin), int(min_period),
                                          int(n_pitch_bins), int(n_bins_per_semitone), float(no_trough_prob), float(tiny), float(log_tiny), c_void_p(log_prob_ptr), c_void_p(voiced_prob_ptr)))

    def pyin_finish_exec(self, states_ptr, n, n_pitch_bins, freqs_ptr, fill_na, f0_ptr, voiced_ptr):
        """states -> f0 and voiced_flag (``include/librosa_amd.h``: lra_pyin_finish_exec); ``fill_na=None`` keeps the best guess in unvoiced frames."""
        _check(self.lib.lra_pyin_finish_exec(self.handle, c_void_p(states_ptr), int(n), int(n_pitch_bins), c_void_p(freqs_ptr), int(fill_na is not None),
                                             0.0 if fill_na is None else float(fill_na), c_void_p(f0_ptr), c_void_p(voiced_ptr)))

    DTW_METRICS = {"euclidean": 0, "sqeuclidean": 1, "cityblock": 2, "cosine": 3}   # the LRA_DTW_* metrics
    DTW_TYPES = {"float32": 0, "float64": 1, "int32": 2, "int64": 3, "uint8": 4}      # what lra_dtw_prepare_exec reads
    DTW_FLAG_NAN, DTW_FLAG_END_INF, DTW_FLAG_ROW_INF, DTW_FLAG_NOT_ORIGIN, DTW_FLAG_BAD_STEP = 1, 2, 4, 8, 16   # the LRA_DTW_FLAG_* bits
    DTW_START_END, DTW_START_ARGMIN = -1, -2

    def dtw_cost_exec(self, x_ptr, y_ptr, dtype, n_features, n, m, metric, c_ptr, work_ptr):
        """The float64 cost matrix of two feature sequences (``include/librosa_amd.h``: lra_dtw_cost_exec).  Returns the flags met (this waits
        for the stream)."""
        flags = c_int(0)
        _check(self.lib.lra_dtw_cost_exec(self.handle, c_void_p(x_ptr), c_void_p(y_ptr), dtype_code(dtype), int(n_features), int(n), int(m), int(metric), c_void_p(c_ptr),
                                          c_void_p(work_ptr), byref(flags)))
        return int(flags.value)

    def dtw_prepare_exec(self, c_ptr, dtype, count, out_ptr, work_ptr):
        """A given cost matrix as float64, and its NaN flag (lra_dtw_prepare_exec); ``out_ptr`` 0: the check alone (float64)."""
        flags = c_int(0)
        _check(self.lib.lra_dtw_prepare_exec(self.handle, c_void_p(c_ptr), int(self.DTW_TYPES[np.dtype(dtype).name]), int(count), c_void_p(out_ptr or None), c_void_p(work_ptr),
                                             byref(flags)))
        return int(flags.value)

    def dtw_accumulate_exec(self, c_ptr, n, m, steps, weights_add, weights_mul, subseq, band, tile, d_ptr, step_idx_ptr):
        """The accumulated cost matrix and the uint8 step indices (lra_dtw_accumulate_exec); ``steps`` int32 (n_steps, 2), the weights float64,
        host arrays; ``band``: None or (band_lo, band_hi)."""
        steps = np.ascontiguousarray(steps, dtype=np.int32)
        weights_add, weights_mul = np.ascontiguousarray(weights_add, dtype=np.float64), np.ascontiguousarray(weights_mul, dtype=np.float64)
        lo, hi = band if band is not None else (0, 0)
        _check(self.lib.lra_dtw_accumulate_exec(self.handle, c_void_p(c_ptr), int(n), int(m), c_void_p(steps.ctypes.data), c_void_p(weights_add.ctypes.data),
                                                c_void_p(weights_mul.ctypes.data), int(steps.shape[0]), int(bool(subseq)), int(band is not None), int(lo), int(hi), int(tile), c_void_p(d_ptr),
                                                c_void_p(step_idx_ptr)))

    def dtw_widen_exec(self, step_idx_ptr, count, out_ptr):
        """uint8 step indices -> int32 (lra_dtw_widen_exec)."""
        _check(self.lib.lra_dtw_widen_exec(self.handle, c_void_p(step_idx_ptr), int(count), c_void_p(out_ptr)))

    def dtw_backtrack_exec(self, d_ptr, step_idx_ptr, steps_i32, n, m, steps, subseq, start, path_ptr, work_ptr):
        """The warping path (lra_dtw_backtrack_exec).  Returns (length, status) (this waits for the stream)."""
        steps = np.ascontiguousarray(steps, dtype=np.int32)
        length, status = c_int64(0), c_int(0)
        _check(self.lib.lra_dtw_backtrack_exec(self.handle, c_void_p(d_ptr or None), c_void_p(step_idx_ptr), int(bool(steps_i32)), int(n), int(m), c_void_p(steps.ctypes.data),
                                               int(steps.shape[0]), int(bool(subseq)), int(start), c_void_p(path_ptr), c_void_p(work_ptr), byref(length), byref(status)))
        return int(length.value), int(status.value)

    RQA_WORK_BYTES = 16 + 16 * 1024   # LRA_RQA_WORK_BYTES

    def rqa_score_exec(self, sim_ptr, dtype, n, m, gap_onset, gap_extend, knight_moves, rows, strip, score_ptr, pointers_ptr):
        """The alignment score matrix (of ``dtype``) and the int8 pointers (``include/librosa_amd.h``: lra_rqa_score_exec)."""
        _check(self.lib.lra_rqa_score_exec(self.handle, c_void_p(sim_ptr), dtype_code(dtype), int(n), int(m), float(gap_onset), float(gap_extend), int(bool(knight_moves)), int(rows),
                                           int(strip), c_void_p(score_ptr), c_void_p(pointers_ptr)))

    def rqa_argmax_exec(self, score_ptr, dtype, count, work_ptr):
        """np.argmax(score) into the work area (lra_rqa_argmax_exec)."""
        _check(self.lib.lra_rqa_argmax_exec(self.handle, c_void_p(score_ptr), dtype_code(dtype), int(count), c_void_p(work_ptr)))

    def rqa_backtrack_exec(self, pointers_ptr, n, m, work_ptr, path_ptr):
        """The alignment path into the last rows of ``path`` (lra_rqa_backtrack_exec).  Returns its length (this waits for the stream)."""
        length = c_int64(0)
        _check(self.lib.lra_rqa_backtrack_exec(self.handle, c_void_p(pointers_ptr), int(n), int(m), c_void_p(work_ptr), c_void_p(path_ptr), byref(length)))
        return int(length.value)

    KNN_MAX_K, KNN_WORK_BYTES = 2048, 64   # LRA_KNN_MAX_K, LRA_KNN_WORK_BYTES
    KNN_MODES = {"connectivity": 0, "distance": 1, "affinity": 2}   # the LRA_KNN_* modes
    KNN_BW_SCALAR, KNN_BW_MATRIX = 0, 6
    KNN_BW_MODES = {"med_k_scalar": 0, "mean_k": 1, "gmean_k": 2, "mean_k_avg": 3, "gmean_k_avg": 4, "mean_k_avg_and_pair": 5}   # the LRA_KNN_BW_* modes
    KNN_STATUS_EMPTY_GRAPH, KNN_STATUS_ROW_EMPTY, KNN_STATUS_NON_POSITIVE = 1, 2, 4   # the LRA_KNN_STATUS_* bits

    def knn_select_exec(self, q_ptr, r_ptr, dtype, n_features, n, m, metric, k, width, skip_zero, rows, tile, count_ptr, index_ptr, distance_ptr):
        """The k nearest candidates of every query frame, each row sorted by index (``include/librosa_amd.h``: lra_knn_select_exec)."""
        _check(self.lib.lra_knn_select_exec(self.handle, c_void_p(q_ptr), c_void_p(r_ptr), dtype_code(dtype), int(n_features), int(n), int(m), int(metric), int(k), int(width),
                                            int(bool(skip_zero)), int(rows), int(tile), c_void_p(count_ptr), c_void_p(index_ptr), c_void_p(distance_ptr)))

    def knn_mutual_exec(self, n, k, count_ptr, index_ptr, distance_ptr, sym, drop_zero, keep_ptr):
        """Which list entries stay (lra_knn_mutual_exec)."""
        _check(self.lib.lra_knn_mutual_exec(self.handle, int(n), int(k), c_void_p(count_ptr), c_void_p(index_ptr), c_void_p(distance_ptr), int(bool(sym)), int(bool(drop_zero)),
                                            c_void_p(keep_ptr)))

    def knn_bandwidth_exec(self, n, k, count_ptr, distance_ptr, keep_ptr, add_self, bandwidth_k, median, dist_to_k_ptr, avg_ptr, work_ptr):
        """The rows' bandwidth statistics and, with ``median``, their nanmedian into the work area (lra_knn_bandwidth_exec).  Returns (status bits,
        the lowest empty row) (this waits for the stream)."""
        status, first = c_int(0), c_int64(0)
        _check(self.lib.lra_knn_bandwidth_exec(self.handle, int(n), int(k), c_void_p(count_ptr), c_void_p(distance_ptr), c_void_p(keep_ptr), int(bool(add_self)), int(bandwidth_k),
                                               int(bool(median)), c_void_p(dist_to_k_ptr), c_void_p(avg_ptr), c_void_p(work_ptr), byref(status), byref(first)))
        return int(status.value), int(first.value)

    def knn_bw_check_exec(self, matrix_ptr, count, work_ptr):
        """The status bits of a bandwidth matrix (lra_knn_bw_check_exec; this waits for the stream)."""
        status = c_int(0)
        _check(self.lib.lra_knn_bw_check_exec(self.handle, c_void_p(matrix_ptr), int(count), c_void_p(work_ptr), byref(status)))
        return int(status.value)

    def knn_emit_exec(self, n, m, k, count_ptr, index_ptr, distance_ptr, keep_ptr, self_link, mode, bw_mode, bw_scalar, bw_on_device, sigma_ptr, matrix_ptr, work_ptr, counts_ptr, indptr_ptr,
                      indices_ptr, data_ptr, dense_ptr):
        """The dense result, or the compressed arrays, of the lists (lra_knn_emit_exec).  Returns the number of stored entries of the compressed
        arrays (this waits for the stream), 0 for a dense result."""
        total = c_int64(0)
        _check(self.lib.lra_knn_emit_exec(self.handle, int(n), int(m), int(k), c_void_p(count_ptr), c_void_p(index_ptr), c_void_p(distance_ptr), c_void_p(keep_ptr), int(bool(self_link)),
                                          int(mode), int(bw_mode), float(bw_scalar), int(bool(bw_on_device)), c_void_p(sigma_ptr), c_void_p(matrix_ptr), c_void_p(work_ptr),
                                          c_void_p(counts_ptr), c_void_p(indptr_ptr), c_void_p(indices_ptr), c_void_p(data_ptr), c_void_p(dense_ptr), byref(total)))
        return int(total.value)

    def knn_dense_exec(self, q_ptr, r_ptr, dtype, n_features, n, m, metric, width, self_link, mode, bw_mode, bw_scalar, bw_on_device, sigma_ptr, matrix_ptr, work_ptr, out_ptr):
        """The transposed dense result where every candidate is kept (lra_knn_dense_exec)."""
        _check(self.lib.lra_knn_dense_exec(self.handle, c_void_p(q_ptr), c_void_p(r_ptr), dtype_code(dtype), int(n_features), int(n), int(m), int(metric), int(width), int(bool(self_link)),
                                           int(mode), int(bw_mode), float(bw_scalar), int(bool(bw_on_device)), c_void_p(sigma_ptr), c_void_p(matrix_ptr), c_void_p(work_ptr), c_void_p(out_ptr)))

    ENHANCE_LDS_MAX, ENHANCE_MAX_REACH = 160 * 1024, 124   # LRA_ENHANCE_LDS_MAX, LRA_ENHANCE_MAX_REACH
    ENHANCE_MODES = {"reflect": 0, "constant": 1, "nearest": 2, "mirror": 3, "wrap": 4}   # the LRA_ENHANCE_* boundary modes
    STACK_MODES = {"constant": 0, "edge": 1, "reflect": 2, "symmetric": 3, "wrap": 4}     # the LRA_STACK_* pad modes
    ENHANCE_TAP = np.dtype([("dr", "<i4"), ("dc", "<i4"), ("w", "<f8")])                  # lra_enhance_tap

    @staticmethod
    def enhance_table_bytes(n_taps, n_filters):
        """LRA_ENHANCE_TABLE_BYTES."""
        return ((int(n_filters) + 1) * 4 + 15) // 16 * 16 + 16 * int(n_taps)

    def path_enhance_exec(self, r_ptr, dtype, channels, h, w, taps, starts, mode, cval, clip, rows, cols, table_ptr, out_ptr):
        """All filters' responses, their maximum and the clip in one launch (``include/librosa_amd.h``: lra_path_enhance_exec).  ``taps``: a host
        array of ``ENHANCE_TAP``; ``starts``: host int32, one more entry than filters."""
        taps = np.ascontiguousarray(taps, dtype=self.ENHANCE_TAP)
        starts = np.ascontiguousarray(starts, dtype=np.int32)
        _check(self.lib.lra_path_enhance_exec(self.handle, c_void_p(r_ptr), dtype_code(dtype), int(channels), int(h), int(w), c_void_p(taps.ctypes.data), c_void_p(starts.ctypes.data),
                                              int(starts.size - 1), int(mode), float(cval), int(bool(clip)), int(rows), int(cols), c_void_p(table_ptr), c_void_p(out_ptr)))

    def shear_exec(self, in_ptr, esize, rows_in, cols_in, period, rows_out, cols_out, factor, axis, out_ptr):
        """The shear of a dense matrix with the lag transforms' pad and slice folded in (lra_shear_exec)."""
        _check(self.lib.lra_shear_exec(self.handle, c_void_p(in_ptr), int(esize), int(rows_in), int(cols_in), int(period), int(rows_out), int(cols_out), int(factor), int(axis),
                                       c_void_p(out_ptr)))

    def stack_memory_exec(self, in_ptr, esize, batch, d, t, n_steps, delay, mode, fill, out_ptr):
        """The delayed copies of [batch][d][t] stacked along d (lra_stack_memory_exec); ``fill``: the constant's bytes as an unsigned integer."""
        _check(self.lib.lra_stack_memory_exec(self.handle, c_void_p(in_ptr), int(esize), int(batch), int(d), int(t), int(n_steps), int(delay), int(mode), int(fill), c_void_p(out_ptr)))

    VITERBI_GENERATIVE, VITERBI_DISCRIMINATIVE, VITERBI_BINARY, VITERBI_LOG = 0, 1, 2, 3   # the LRA_VITERBI_* kinds
    VITERBI_FLAG_NEGATIVE, VITERBI_FLAG_ABOVE_ONE, VITERBI_FLAG_COLUMN_SUM = 1, 2, 4       # the LRA_VITERBI_FLAG_* bits

    def viterbi_prep_exec(self, prob_ptr, dtype, kind, chains, n_states, n_steps, eps, log_marginal_ptr, n_labels, log_prob_ptr, work_ptr):
        """prob -> the float64 log table [chain][step][state] (``include/librosa_amd.h``: lra_viterbi_prep_exec).  Returns the range flags met
        (this waits for the stream)."""
        flags = c_int(0)
        _check(self.lib.lra_viterbi_prep_exec(self.handle, c_void_p(prob_ptr), dtype_code(dtype), int(kind), int(chains), int(n_states), int(n_steps), float(eps),
                                              c_void_p(log_marginal_ptr or None), int(n_labels), c_void_p(log_prob_ptr), c_void_p(work_ptr), byref(flags)))
        return int(flags.value)

    def viterbi_exec(self, log_prob_ptr, chains, n_states, n_steps, log_trans_ptr, log_p_init_ptr, n_tables, threshold, n_pred, pred_k_ptr, pred_lt_ptr, pred_n_ptr, ptr_ptr, states_ptr,
                     logp_ptr):
        """The decode of every chain (``include/librosa_amd.h``: lra_viterbi_exec)."""
        _check(self.lib.lra_viterbi_exec(self.handle, c_void_p(log_prob_ptr), int(chains), int(n_states), int(n_steps), c_void_p(log_trans_ptr or None), c_void_p(log_p_init_ptr),
                                         int(n_tables), float(threshold), int(n_pred), c_void_p(pred_k_ptr or None), c_void_p(pred_lt_ptr or None), c_void_p(pred_n_ptr or None),
                                         c_void_p(ptr_ptr), c_void_p(states_ptr), c_void_p(logp_ptr)))

    PITCH_REF_MAX, PITCH_REF_ROW, PITCH_REF_SCALAR = 0, 1, 2   # the LRA_PITCH_REF_* values

    def piptrack_exec(self, s_ptr, batch, n_bins, n_frames, strides, dtype, bin_lo, bin_hi, ref_mode, threshold, ref_row_ptr, ref_scalar, sr, n_fft, pitches_ptr, mags_ptr, out_strides):
        """The dense pitch tracker (``include/librosa_amd.h``: lra_piptrack_exec); ``strides`` / ``out_strides``: (batch, bin, frame) in elements."""
        _check(self.lib.lra_piptrack_exec(self.handle, c_void_p(s_ptr), int(batch), int(n_bins), int(n_frames), int(strides[0]), int(strides[1]), int(strides[2]), dtype_code(dtype),
                                          int(bin_lo), int(bin_hi), int(ref_mode), float(threshold), c_void_p(ref_row_ptr or None), float(ref_scalar), float(sr), int(n_fft),
                                          c_void_p(pitches_ptr), c_void_p(mags_ptr), int(out_strides[0]), int(out_strides[1]), int(out_strides[2])))

    def tuning_work_bytes(self, batch, n_frames, masked_bins, dtype):
        return int(self.lib.lra_tuning_work_bytes(int(batch), int(n_frames), int(masked_bins), dtype_code(dtype)))

    def tuning_exec(self, s_ptr, batch, n_bins, n_frames, strides, dtype, bin_lo, bin_hi, ref_mode, threshold, ref_row_ptr, ref_scalar, sr, n_fft, edges_ptr, n_hist, bins_per_octave,
                    work_ptr, out_ptr):
        """Peaks, their median magnitude and the tuning histogram in one native call (lra_tuning_exec); ``out``: int64 [n_hist + 2] on the device."""
        _check(self.lib.lra_tuning_exec(self.handle, c_void_p(s_ptr), int(batch), int(n_bins), int(n_frames), int(strides[0]), int(strides[1]), int(strides[2]), dtype_code(dtype),
                                        int(bin_lo), int(bin_hi), int(ref_mode), float(threshold), c_void_p(ref_row_ptr or None), float(ref_scalar), float(sr), int(n_fft),
                                        c_void_p(edges_ptr), int(n_hist), float(bins_per_octave), c_void_p(work_ptr), c_void_p(out_ptr)))

    def pitch_tuning_exec(self, freq_ptr, n, dtype, edges_ptr, n_hist, bins_per_octave, out_ptr):
        """The tuning histogram of a frequency array (lra_pitch_tuning_exec); ``out``: int64 [n_hist + 2] on the device."""
        _check(self.lib.lra_pitch_tuning_exec(self.handle, c_void_p(freq_ptr or None), int(n), dtype_code(dtype), c_void_p(edges_ptr), int(n_hist), float(bins_per_octave), c_void_p(out_ptr)))

    def magnitude_exec(self, d_ptr, mag_ptr, count, dtype):
        _check(self.lib.lra_magnitude_exec(self.handle, c_void_p(d_ptr), c_void_p(mag_ptr), count, dtype_code(dtype)))

    def magphase_exec(self, d_ptr, is_complex, mag_ptr, phase_ptr, count, power, dtype):
        _check(self.lib.lra_magphase_exec(self.handle, c_void_p(d_ptr), int(bool(is_complex)), c_void_p(mag_ptr), c_void_p(phase_ptr), count, float(power), dtype_code(dtype)))

    def hpss_exec(self, mag_ptr, d_ptr, out_h_ptr, out_p_ptr, batch, n_frames, n_bins, win_harm, win_perc, power, margin_harm, margin_perc, want_mask, dtype):
        _check(self.lib.lra_hpss_exec(self.handle, c_void_p(mag_ptr), c_void_p(d_ptr or None), c_void_p(out_h_ptr), c_void_p(out_p_ptr), batch, n_frames, int(n_bins), int(win_harm), int(win_perc),
                                      float(power), float(margin_harm), float(margin_perc), int(bool(want_mask)), dtype_code(dtype)))

    def memset(self, ptr, value, nbytes):
        _check(self.lib.lra_memset(self.handle, c_void_p(ptr), int(value), int(nbytes)))

    def griffinlim_init(self, u_ptr, s_ptr, angles_ptr, count, dtype):
        _check(self.lib.lra_griffinlim_init(self.handle, c_void_p(u_ptr), c_void_p(s_ptr), c_void_p(angles_ptr), count, dtype_code(dtype)))

    @staticmethod
    def _pcg64_state4(state, inc):
        m = (1 << 64) - 1
        return (ctypes.c_uint64 * 4)((int(state) >> 64) & m, int(state) & m, (int(inc) >> 64) & m, int(inc) & m)

    def pcg64_random_exec(self, state, inc, offset, out_ptr, count):
        """``np.random.Generator(PCG64)`` with the 128-bit ``state`` / ``inc`` of its ``bit_generator.state["state"]``: draws ``offset .. offset + count`` of ``random()`` (float64, device)."""
        _check(self.lib.lra_pcg64_random_exec(self.handle, self._pcg64_state4(state, inc), int(offset), c_void_p(out_ptr), int(count)))

    def griffinlim_init_pcg64(self, state, inc, s_ptr, angles_ptr, batch, n_bins, n_frames, dtype):
        _check(self.lib.lra_griffinlim_init_pcg64(self.handle, self._pcg64_state4(state, inc), c_void_p(s_ptr), c_void_p(angles_ptr), int(batch), int(n_bins), int(n_frames), dtype_code(dtype)))

    def griffinlim_update(self, rebuilt_ptr, tprev_ptr, s_ptr, angles_ptr, count, dtype, coef, eps, normalize=True):
        _check(self.lib.lra_griffinlim_update(self.handle, c_void_p(rebuilt_ptr), c_void_p(tprev_ptr) if tprev_ptr else None, c_void_p(s_ptr), c_void_p(angles_ptr), count, dtype_code(dtype),
                                              float(coef), float(eps), int(bool(normalize))))

    def probe_stream(self, direction, in_ptr, out_ptr, batch, rows_per_clip, n_fft, hop, clip_samples, strip_rows=0, waves_per_cu=0, row_pitch_bytes=0, piece_bytes=8):
        """The transform's access stream without its arithmetic (measurement aid; ``include/librosa_amd.h``)."""
        _check(self.lib.lra_probe_stream_pitched(self.handle, int(direction), c_void_p(in_ptr), c_void_p(out_ptr), batch, rows_per_clip, n_fft, hop, clip_samples, strip_rows, waves_per_cu,
                                                 int(row_pitch_bytes), int(piece_bytes)))

    def probe_stream_window(self, in_ptr, out_ptr, batch, rows_per_clip, n_fft, hop, clip_samples, strip_rows, waves_per_cu):
        """The forward access stream with the strips dealt out in address order to persistent waves (``include/librosa_amd.h``)."""
        _check(self.lib.lra_probe_stream_window(self.handle, c_void_p(in_ptr), c_void_p(out_ptr), batch, rows_per_clip, n_fft, hop, clip_samples, int(strip_rows), int(waves_per_cu)))

    def transpose(self, src_ptr, dst_ptr, batch, rows, cols, elem_bytes):
        _check(self.lib.lra_transpose(self.handle, c_void_p(src_ptr), c_void_p(dst_ptr), batch, rows, cols, elem_bytes))


_contexts = {}
_ctx_lock = threading.Lock()


COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """RCCL unique id for a new communicator (rank 0 calls this; the host program distributes the bytes)."""
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    _check(load_library().lra_comm_unique_id(buf))
    return buf.raw


class Comm:
    """Native RCCL communicator of one rank (``include/librosa_amd.h``: ``lra_comm_*``), bound to a context's device and stream."""

    def __init__(self, ctx, rank, n_ranks, unique_id: bytes):
        self.ctx, self.rank, self.n_ranks = ctx, int(rank), int(n_ranks)
        self.lib = ctx.lib
        h = c_void_p()
        buf = ctypes.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        _check(self.lib.lra_comm_init(ctx.handle, self.rank, self.n_ranks, buf, byref(h)))
        self.handle = h

    def allgather(self, send_ptr, recv_ptr, bytes_per_rank):
        _check(self.lib.lra_comm_allgather(self.handle, c_void_p(send_ptr), c_void_p(recv_ptr), int(bytes_per_rank)))

    def allgatherv(self, send_ptr, recv_ptr, bytes_per_rank, recv_offsets):
        """Unequal shards: rank r's ``bytes_per_rank[r]`` bytes land at ``recv_ptr + recv_offsets[r]`` on every rank (one grouped broadcast per rank)."""
        n = self.n_ranks
        if len(bytes_per_rank) != n or len(recv_offsets) != n:
            raise ParameterError(f"allgatherv: size / offset tables must have one entry per rank ({n})")
        sizes = (c_size_t * n)(*[int(v) for v in bytes_per_rank])
        offs = (c_size_t * n)(*[int(v) for v in recv_offsets])
        _check(self.lib.lra_comm_allgatherv(self.handle, c_void_p(send_ptr) if send_ptr else None, c_void_p(recv_ptr), sizes, offs))

    def close(self):
        if self.handle:
            self.lib.lra_comm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_devices():
    """Devices the NumPy drop-in spreads the clips of one call over, inside ONE process (a thread, a context and a host pipeline per
    device; ctypes releases the GIL during native calls).  Opt-in (a plain NumPy call must not wake contexts on every GPU of
    the node, least of all under a one-process-per-GPU launcher that this library does not know -- SLURM, MPI, a multiprocessing pool):
    by default a call stays on the process's own device (``get_context()``: ``LIBROSA_AMD_DEVICE`` / ``LOCAL_RANK``, else 0);
    ``LRA_DEVICES=all`` = every visible device, ``LRA_DEVICES=0,2`` = those."""
    n = device_count()
    if n <= 0:
        return [0]
    spec = os.environ.get("LRA_DEVICES", "").strip().lower()
    if spec == "":
        return [get_context().device]
    if spec == "all":
        return list(range(n))
    try:
        devs = [int(t) for t in spec.split(",") if t.strip()]
    except ValueError:
        raise ParameterError(f"LRA_DEVICES={spec!r}: expected comma-separated device indices or 'all'")
    bad = [d for d in devs if not 0 <= d < n]
    if bad:
        raise ParameterError(f"LRA_DEVICES names device(s) {bad}, but {n} device(s) are visible")
    return devs or [0]


def get_context(device=None):
    """Shared per-device context.  ``device=None`` -> LOCAL_RANK's device under torchrun, else 0."""
    if device is None:
        device = int(os.environ.get("LIBROSA_AMD_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        n = device_count()
        if n > 0:
            device %= n
    with _ctx_lock:
        ctx = _contexts.get(device)
        if ctx is None:
            ctx = Context(device)
            _contexts[device] = ctx
    return ctx
