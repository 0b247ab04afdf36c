"""Producer / consumer fused mel kernel (librosa_amd/csrc/lra_kernels_pc.h): every phase of the consumer's eight-frame output tile.

The consumer keeps the tile slot in a scalar register where rows start 0 or 16 bytes into a 32-byte piece (n_frames % 4 == 0) and per lane
otherwise; the first and last bursts of a producer slot are partial.  These cases walk n_frames % 8 through 0..7, producer slots whose length is
not a multiple of eight, clips that end inside a tile and 120 / 125 / 128 bands: bit for bit against the one-wave body in the simulator, and on
the device against the oracle, against the one-wave kernel, and batch against per-clip.  librosa/feature/spectral.py:2158-2160."""
import numpy as np
import pytest

import hostsim_util as H
import stft_oracle as O

# (frames of a clip at hop 512, centred: 1 + n // 512) -> n_frames % 8 = 0..7; producer-slot lengths (iters) that are not multiples of 8
_SIM_CASES = [(16 + k, it, nm) for k, it, nm in zip(range(8), (3, 5, 9, 10, 11, 6, 13, 7), (128, 125, 120, 128, 125, 120, 128, 128))]


_SIM_ITERS = {nf: it for nf, it, _ in _SIM_CASES}


def _check_diag(d):
    assert d["races"] == 0 and d["uninit"] == 0, d


@pytest.mark.parametrize("n_frames,iters,n_mels", _SIM_CASES)
def test_sim_consumer_tile_phases(n_frames, iters, n_mels, monkeypatch):
    n = (n_frames - 1) * 512 + 37
    rng = np.random.default_rng(n_frames * 100 + iters)
    y = rng.standard_normal((2, n)).astype(np.float32)
    win = O.get_window("hann", 2048)
    B = O.mel(sr=22050, n_fft=2048, n_mels=n_mels)
    M4, d4 = H.stft(y, 2048, 512, win, mode=4, power=2.0, mel_basis=B, iters_per_wg=iters)
    monkeypatch.setenv("LRA_SIM_PC", "1")
    Mp, dp = H.stft(y, 2048, 512, win, mode=4, power=2.0, mel_basis=B, iters_per_wg=iters)
    assert Mp is not None and dp["NT"] == 192, dp
    _check_diag(dp)
    assert Mp.shape[-1] == n_frames and not np.isnan(Mp).any()
    assert np.array_equal(Mp, M4)
    Mref = O.melspectrogram(y=y, sr=22050, n_fft=2048, hop_length=512, power=2.0, n_mels=n_mels)
    assert np.all(np.abs(Mp - Mref) <= 1e-5 * np.abs(Mref) + 1e-5 * Mref.max())


@pytest.mark.gpu
@pytest.mark.parametrize("n_frames,n_mels", [(nf, nm) for nf, _, nm in _SIM_CASES] + [(1292, 128), (1293, 125)])
def test_gpu_consumer_tile_phases(n_frames, n_mels):
    import librosa_amd as L
    import torch
    ctx = L.get_context(0)
    n = (n_frames - 1) * 512 + 37
    y = O.config_input(3, n=n)
    ref = O.melspectrogram(y=y, sr=22050, n_fft=2048, hop_length=512, n_mels=n_mels)
    yt = torch.from_numpy(y).to("cuda:0")
    try:
        outs = []
        for pc in (0, 1):
            ctx.set_option("mel_pc", pc)
            M = L.feature.melspectrogram(y=yt, sr=22050, n_fft=2048, hop_length=512, n_mels=n_mels).cpu().numpy()
            assert M.shape == ref.shape and not np.isnan(M).any()
            assert np.all(np.abs(M - ref) <= 1e-4 * np.abs(ref)), (pc, float(np.max(np.abs(M - ref) / np.abs(ref))))
            outs.append(M)
        assert np.all(np.abs(outs[1] - outs[0]) <= 2e-5 * np.abs(outs[0]))
        for i in range(3):
            Mi = L.feature.melspectrogram(y=yt[i], sr=22050, n_fft=2048, hop_length=512, n_mels=n_mels).cpu().numpy()
            assert np.array_equal(Mi, outs[1][i]), i
        # once more at the simulator case's own producer-slot length (the auto rule gives these short clips slots of at most four frames)
        if n_frames in _SIM_ITERS:
            ctx.set_option("stft_iters", _SIM_ITERS[n_frames])
            forced = []
            for pc in (0, 1):
                ctx.set_option("mel_pc", pc)
                M = L.feature.melspectrogram(y=yt, sr=22050, n_fft=2048, hop_length=512, n_mels=n_mels).cpu().numpy()
                assert M.shape == ref.shape and not np.isnan(M).any()
                assert np.all(np.abs(M - ref) <= 1e-4 * np.abs(ref)), (pc, _SIM_ITERS[n_frames], float(np.max(np.abs(M - ref) / np.abs(ref))))
                forced.append(M)
            assert np.all(np.abs(forced[1] - forced[0]) <= 2e-5 * np.abs(forced[0]))
    finally:
        ctx.set_option("mel_pc", 1)  # (the library's default)
        ctx.set_option("stft_iters", 0)


@pytest.mark.gpu
def test_gpu_consumer_batch_512_clips():
    """512 clips x 30 s in one launch (twice the bench's batch): four sampled clips at the pure-relative bar, each equal to the clip run alone."""
    import librosa_amd as L
    import torch
    ctx = L.get_context(0)
    ctx.set_option("mel_pc", 1)
    yt = torch.from_numpy(O.config_input(512, n=661500)).to("cuda:0")
    M = L.feature.melspectrogram(y=yt, sr=22050, n_fft=2048, hop_length=512, n_mels=128)
    assert not bool(torch.isnan(M).any())
    for i in (0, 173, 384, 511):
        ref = O.melspectrogram(y=yt[i].cpu().numpy(), sr=22050, n_fft=2048, hop_length=512, n_mels=128)
        got = M[i].cpu().numpy()
        assert np.all(np.abs(got - ref) <= 1e-4 * np.abs(ref)), i
        assert np.array_equal(L.feature.melspectrogram(y=yt[i], sr=22050, n_fft=2048, hop_length=512, n_mels=128).cpu().numpy(), got), i
