"""Producer / consumer fused mel kernel (librosa_amd/csrc/lra_kernels_pc.h): the producer wave's own edges.

The producer takes its lane index by a mask, derives the sixteen power-row store addresses from one base by XOR (v2_pw_addr_xor) and forms
|X[k]|^2, |X[M-k]|^2 of a pair slot from the transposed split (split_pair_pow2); lane 0's pair slots are arranged differently from every
other lane's.  These cases walk a producer slot of one frame, a slot-1 tail that lies wholly past the clip, hop n_fft / 4 with |X|^2 and hop
n_fft / 8 with |X| and |X|^2 (the HD = 8 instance), an input whose energy sits in the bins of lane 0's two butterflies (0 and s/2: bins 64 j),
the per-lane tile form (n_frames = 1293) and the clip-edge load path (pad_mode="reflect"): bit for bit against the one-wave body in the
simulator, and on the device against the oracle, against the one-wave kernel, and batch against per-clip.  librosa/feature/spectral.py:2158-2160."""
import numpy as np
import pytest

import hostsim_util as H
import stft_oracle as O

SR, N_FFT = 22050, 2048
# (hop, power): hop n_fft / 4 serves |X|^2 only; hop n_fft / 8 serves |X| and |X|^2
_HOP_POWER = [(512, 2.0), (256, 1.0), (256, 2.0)]
_SIM_CASES = [(nf, it, hop, p) for hop, p in _HOP_POWER for nf in (1, 2, 3, 5) for it in (1, 2, 3)]


def _n_samples(n_frames, hop):
    return (n_frames - 1) * hop + 37


def _lane0_input(batch, n):
    """0.1 x seeded noise + fifteen 0.05-amplitude sines at exactly bins 64 j, j = 1 .. 15 (butterflies 0 and s/2 of the last pass: lane 0's)."""
    rng = np.random.default_rng(6464)
    t = np.arange(n, dtype=np.float64)
    y = 0.1 * rng.standard_normal((batch, n))
    for j in range(1, 16):
        y += 0.05 * np.sin(2 * np.pi * (64 * j) * t / N_FFT + 0.3 * j)[None, :]
    return y.astype(np.float32)


def _check_diag(d):
    assert d["races"] == 0 and d["uninit"] == 0, d


def _sim_pair(y, hop, power, window, iters, monkeypatch):
    win = O.get_window(window, N_FFT)
    B = O.mel(sr=SR, n_fft=N_FFT, n_mels=128)
    monkeypatch.delenv("LRA_SIM_PC", raising=False)
    M4, _ = H.stft(y, N_FFT, hop, win, mode=4, power=power, mel_basis=B, iters_per_wg=iters)
    monkeypatch.setenv("LRA_SIM_PC", "1")
    Mp, dp = H.stft(y, N_FFT, hop, win, mode=4, power=power, mel_basis=B, iters_per_wg=iters)
    assert M4 is not None and Mp is not None and dp["NT"] == 192, dp
    _check_diag(dp)
    assert not np.isnan(Mp).any()
    assert np.array_equal(Mp, M4)
    Mref = O.melspectrogram(y=y, sr=SR, n_fft=N_FFT, hop_length=hop, power=power, n_mels=128, window=window)
    assert Mp.shape == Mref.shape
    err = np.abs(Mp - Mref) - (1e-5 * np.abs(Mref) + 1e-5 * Mref.max())
    print(f"sim hop {hop} power {power} window {window} iters {iters}: max excess over the bar {float(err.max()):.3g}")
    assert np.all(err <= 0)


@pytest.mark.parametrize("n_frames,iters,hop,power", _SIM_CASES)
def test_sim_producer_slot_edges(n_frames, iters, hop, power, monkeypatch):
    rng = np.random.default_rng(1000 * n_frames + 10 * iters + hop)
    y = rng.standard_normal((2, _n_samples(n_frames, hop))).astype(np.float32)
    _sim_pair(y, hop, power, "hann", iters, monkeypatch)


@pytest.mark.parametrize("hop,power", _HOP_POWER)
def test_sim_lane0_pairing(hop, power, monkeypatch):
    """Boxcar window: each sine stays in its own bin 64 j, so a wrong lane-0 pairing or store address moves its energy to another band."""
    y = _lane0_input(2, _n_samples(5, hop))
    _sim_pair(y, hop, power, "boxcar", 3, monkeypatch)


# ---- device ------------------------------------------------------------------------------------------------------------------------
# (n_frames, hop, power, window, pad_mode, input)
_GPU_CASES = [(nf, hop, p, "hann", "constant", "config") for hop, p in _HOP_POWER for nf in (1, 2, 3, 5)]
_GPU_CASES += [(5, hop, p, "boxcar", "constant", "lane0") for hop, p in _HOP_POWER]
_GPU_CASES += [(1293, 512, 2.0, "hann", "constant", "config"), (1293, 512, 2.0, "boxcar", "constant", "lane0"), (12, 512, 2.0, "hann", "reflect", "config"),
               (12, 256, 1.0, "hann", "reflect", "config")]


def _sim_iters(n_frames, hop, power, window, pad_mode, kind):
    """The producer-slot lengths at which the simulator half runs this device case."""
    if pad_mode != "constant":
        return []
    if kind == "lane0":
        return [3] if n_frames == 5 else []
    return sorted({it for nf, it, h, p in _SIM_CASES if (nf, h, p) == (n_frames, hop, power)}) if window == "hann" else []


@pytest.mark.gpu
@pytest.mark.parametrize("n_frames,hop,power,window,pad_mode,kind", _GPU_CASES)
def test_gpu_producer_paths(n_frames, hop, power, window, pad_mode, kind):
    import librosa_amd as L
    import torch
    ctx = L.get_context(0)
    n = _n_samples(n_frames, hop)
    y = O.config_input(3, n=n) if kind == "config" else _lane0_input(3, n)
    kw = dict(sr=SR, n_fft=N_FFT, hop_length=hop, n_mels=128, power=power, window=window, pad_mode=pad_mode)
    ref = O.melspectrogram(y=y, **kw)
    assert ref.shape[-1] == n_frames
    yt = torch.from_numpy(y).to("cuda:0")
    try:
        outs = []
        for pc in (0, 1):
            ctx.set_option("mel_pc", pc)
            M = L.feature.melspectrogram(y=yt, **kw).cpu().numpy()
            assert M.shape == ref.shape and not np.isnan(M).any()
            rel = float(np.max(np.abs(M - ref) / np.abs(ref)))
            print(f"mel_pc {pc}: max rel err against the oracle {rel:.3g}")
            assert np.all(np.abs(M - ref) <= 1e-4 * np.abs(ref)), (pc, rel)
            outs.append(M)
        both = float(np.max(np.abs(outs[1] - outs[0]) / np.abs(outs[0])))
        print(f"mel_pc 1 against 0: max rel diff {both:.3g}")
        assert np.all(np.abs(outs[1] - outs[0]) <= 2e-5 * np.abs(outs[0])), both
        for i in range(3):
            Mi = L.feature.melspectrogram(y=yt[i], **kw).cpu().numpy()
            assert np.array_equal(Mi, outs[1][i]), i
        # once more at the simulator cases' own producer-slot lengths for this clip (test_sim_producer_slot_edges, test_sim_lane0_pairing)
        for iters in _sim_iters(n_frames, hop, power, window, pad_mode, kind):
            ctx.set_option("stft_iters", iters)
            forced = []
            for pc in (0, 1):
                ctx.set_option("mel_pc", pc)
                M = L.feature.melspectrogram(y=yt, **kw).cpu().numpy()
                assert M.shape == ref.shape and not np.isnan(M).any()
                rel = float(np.max(np.abs(M - ref) / np.abs(ref)))
                print(f"stft_iters {iters} mel_pc {pc}: max rel err against the oracle {rel:.3g}")
                assert np.all(np.abs(M - ref) <= 1e-4 * np.abs(ref)), (iters, pc, rel)
                forced.append(M)
            assert np.all(np.abs(forced[1] - forced[0]) <= 2e-5 * np.abs(forced[0])), iters
    finally:
        ctx.set_option("mel_pc", 1)  # (the library's default)
        ctx.set_option("stft_iters", 0)
