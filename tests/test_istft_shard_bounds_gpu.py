"""The sample-sharded host istft (core/spectrum.py: run_samples -- one long NumPy spectrogram rebuilt by output-sample ranges when there are
fewer clips than devices) must hand lra_istft_exec_host only memory inside the spectrogram: `batch` items of `n_frames` frames from the pointer
it passes.  It used to pass a pointer `fa` frames into the array together with all `n_total` frames per item, so the staging copy read `fa`
frames past the array's end.  The calls are checked BEFORE they reach the library, so an offending call raises here instead of reading."""
import numpy as np
import pytest

import golden_cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("clips", [1, 2])
def test_sharded_istft_reads_inside_the_spectrogram(monkeypatch, clips):
    import librosa_amd as L
    from librosa_amd import _native
    from librosa_amd.core import spectrum

    n_fft, hop = 512, 128
    y = golden_cases.make_signal("noise", 22050, 5, (clips,))
    monkeypatch.setenv("LRA_DEVICES", "0")
    D = L.stft(y, n_fft=n_fft, hop_length=hop)
    whole = L.istft(D, n_fft=n_fft, hop_length=hop)
    Dt = np.swapaxes(D, -1, -2)
    assert Dt.flags["C_CONTIGUOUS"]
    lo, hi = Dt.ctypes.data, Dt.ctypes.data + Dt.nbytes
    n_bins = n_fft // 2 + 1
    seen = []
    orig = _native.Context.istft_exec_host

    def checked(self, plan, d_ptr, batch, n_frames, n_used, *rest):
        end = d_ptr + batch * n_frames * n_bins * D.itemsize
        seen.append((d_ptr - lo, end - lo))
        assert lo <= d_ptr and end <= hi, f"istft_exec_host would read {end - hi} bytes past the spectrogram"
        return orig(self, plan, d_ptr, batch, n_frames, n_used, *rest)

    monkeypatch.setattr(_native.Context, "istft_exec_host", checked)
    monkeypatch.setattr(spectrum, "_MULTI_DEVICE_MIN_BYTES", 0)
    monkeypatch.setattr(spectrum, "_FRAME_SHARD_MIN_FRAMES", 8)
    monkeypatch.setenv("LRA_DEVICES", "0,0,0")
    assert spectrum._istft_sample_shards(whole.shape[-1], D.shape[-1], clips, 1 << 40, n_fft, hop, True) is not None
    got = L.istft(D, n_fft=n_fft, hop_length=hop)
    assert len(seen) >= 3 and any(start > 0 for start, _ in seen)  # the sharded route ran, with shards that begin inside the array
    assert np.array_equal(got, whole)
