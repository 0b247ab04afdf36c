"""The C-ABI library loads and exports every symbol include/librosa_amd.h declares, with one error slot for all of its translation units
(CPU: no compute calls)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "librosa_amd.h")


def _declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(lra_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_expected_surface():
    names = _declared_symbols()
    for must in ("lra_ctx_create", "lra_stft_plan_create", "lra_stft_exec", "lra_spectrogram_exec", "lra_mel_plan_create", "lra_melspectrogram_exec",
                 "lra_mel_apply_exec", "lra_istft_plan_create", "lra_istft_exec", "lra_transpose", "lra_last_error"):
        assert must in names
    assert len(names) >= 30


def test_library_exports_every_declared_symbol():
    from librosa_amd import _native

    assert os.path.exists(_native.LIB_PATH), "build the library first: python -c 'import __graft_entry__ as g; g.build()'"
    # the load order of _native.load_library: torch's HIP runtime first, so that the library binds to it.  Loaded the other way round,
    # the process holds two HIP runtimes and torch finds no device in every later test of the same session.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = ctypes.CDLL(_native.LIB_PATH)
    missing = [n for n in _declared_symbols() if not hasattr(lib, n)]
    assert not missing, f"declared in the header but not exported: {missing}"
    # and the Python binding covers the whole header
    unbound = [n for n in _declared_symbols() if n not in _native.SIGNATURES]
    assert not unbound, f"declared in the header but not bound in _native.SIGNATURES: {unbound}"
    extra = [n for n in _native.SIGNATURES if n not in _declared_symbols()]
    assert not extra, f"bound but not declared in the header: {extra}"


def test_no_device_means_loud_failure():
    """Without a GPU every compute entry point must fail loudly (no CPU fallback)."""
    import numpy as np

    import librosa_amd as L

    if L.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(L.NativeError):
        L.stft(np.zeros(4096, np.float32))
    with pytest.raises(L.NativeError):
        L.feature.melspectrogram(y=np.zeros(4096, np.float32))
    with pytest.raises(L.NativeError):
        L.istft(np.zeros((1025, 4), np.complex64))


def test_product_never_imports_the_oracle():
    """The oracle and the host simulator are test infrastructure: nothing under librosa_amd/ may import,
    include or load them."""
    pkg = os.path.join(ROOT, "librosa_amd")
    bad = re.compile(r"^\s*(import|from)\s+(stft_oracle|ref_shim|golden_cases|hostsim_util)\b|#\s*include\s+\"[^\"]*(oracle|tests)/|_hostsim\.so|oracle/", re.M)
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip")):
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                code = "\n".join(line for line in txt.splitlines() if not line.lstrip().startswith(("//", "#  ", "*", '"""')))
                m = bad.search(code)
                assert m is None, (os.path.join(dirpath, f), m.group(0))


# one entry point of each family whose C entry points are defined beside their kernels (csrc/lra_<feature>_inst.hip), not in lra_api.hip
_FEATURE_UNIT_ENTRY_POINTS = ("lra_tempogram_exec", "lra_beat_exec", "lra_peak_pick_exec", "lra_prev_minimum_exec", "lra_chroma_exec", "lra_piptrack_exec", "lra_tuning_exec",
                              "lra_viterbi_exec", "lra_dtw_cost_exec", "lra_rqa_score_exec", "lra_knn_select_exec", "lra_yin_exec", "lra_pyin_obs_exec")


@pytest.mark.parametrize("name", _FEATURE_UNIT_ENTRY_POINTS)
def test_one_error_slot_across_translation_units(name):
    """A failure raised in a feature unit is what lra_last_error() (defined in lra_api.hip) reports, and a later failure in the API unit
    replaces it: the library has one thread-local error slot, not one per translation unit.  No device needed: a null context fails first."""
    from librosa_amd import _native

    lib = _native.load_library()
    _, argtypes = _native.SIGNATURES[name]
    assert lib.lra_device_count(None) == _native.LRA_EINVAL and lib.lra_last_error() == b"null count"  # the slot holds an API-unit message
    assert getattr(lib, name)(*(t() for t in argtypes)) == _native.LRA_EINVAL  # every argument zero / null
    assert lib.lra_last_error() == b"null context"
    assert lib.lra_device_count(None) == _native.LRA_EINVAL and lib.lra_last_error() == b"null count"
    assert lib.lra_stft_plan_create(*(t() for t in _native.SIGNATURES["lra_stft_plan_create"][1])) == _native.LRA_EINVAL
    assert lib.lra_last_error() == b"null context"
