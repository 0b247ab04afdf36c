"""The fused STFT, mel and ISTFT kernels at every launch geometry, on the device (cases: tests/geometry_cases.py).

A frame's spectrum or mel column and an output sample of the inverse depend on the input alone, not on the slot, strip or workgroup that
computed them, and within one kernel instance the instruction sequence per frame is the same for every geometry.  So for every
``stft_iters``, ``istft_strip_groups`` and ``xcd_remap`` the result equals the default result bit for bit (``torch.equal``); the default
result is compared with the oracle at the family's bar of tests/test_gpu_parity.py, holds no NaN, and clip i of the batch equals clip i
computed alone.  Result buffers start as NaN bit patterns, so a frame or sample that a geometry leaves unwritten shows.

The library's finite check stays on: a hand-over timeout of the producer / consumer kernel (bit 1 of the sticky flag) raises."""
import contextlib

import numpy as np
import pytest

import geometry_cases as G
import stft_oracle as O
from test_gpu_parity import _istft_close, _mel_close, _stft_close, _wss_for

pytestmark = pytest.mark.gpu

SR = 22050


@pytest.fixture(scope="module")
def L():
    import librosa_amd

    assert librosa_amd.device_count() > 0, "no HIP device: the product has no CPU fallback"
    return librosa_amd


@pytest.fixture(autouse=True)
def _poisoned_results(monkeypatch):
    from librosa_amd import _arrays

    monkeypatch.setattr(_arrays, "POISON_OUTPUTS", True)


@contextlib.contextmanager
def _options(ctx, **opts):
    """Family options for the duration of a test; every geometry and selection option goes back to the library's default afterwards."""
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k, v in G.OPTION_DEFAULTS.items():
            ctx.set_option(k, v)


def _n_cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _signal(batch, n, dtype, seed):
    return np.random.default_rng(seed).standard_normal((batch, n)).astype(dtype) * 0.25


def _no_nan(x):
    import torch

    return not bool(torch.isnan(x).any())


def _group(points):
    groups = {}
    for key, geo in points:
        groups.setdefault(key, []).append(geo)
    return sorted(groups.items())


# ---- forward ------------------------------------------------------------------------------------------------------------------------
def _forward_call(L, fam, yt):
    if fam.kind == "stft":
        return L.stft(yt, n_fft=fam.n_fft, hop_length=fam.hop)
    if fam.kind == "power":
        return L._spectrogram(y=yt, n_fft=fam.n_fft, hop_length=fam.hop, power=fam.power)[0]
    return L.feature.melspectrogram(y=yt, sr=SR, n_fft=fam.n_fft, hop_length=fam.hop, n_mels=fam.n_mels, power=fam.power)


def _forward_oracle(fam, y):
    if fam.kind == "stft":
        return O.stft(y, n_fft=fam.n_fft, hop_length=fam.hop)
    if fam.kind == "power":
        return O.spectrogram(y=y, n_fft=fam.n_fft, hop_length=fam.hop, power=fam.power)[0]
    return O.melspectrogram(y=y, sr=SR, n_fft=fam.n_fft, hop_length=fam.hop, n_mels=fam.n_mels, power=fam.power)


def _forward_close(fam, got, ref):
    """The family's bar in tests/test_gpu_parity.py: _stft_close, test_golden_case's |X|^p bar, _mel_close, and the pure-relative mel bar of
    test_producer_consumer_mel_kernel (noise-floored input)."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    if fam.bar == "stft":
        return _stft_close(got, ref)
    if fam.bar == "power":
        if got.dtype == np.float64:
            return np.all(np.abs(got - ref) <= 1e-11 * ref.max())
        return np.all(np.abs(got - ref) <= 1e-4 * np.abs(ref) + 1e-5 * ref.max())
    if fam.bar == "mel-rel":
        return np.all(np.abs(got - ref) <= 1e-4 * np.abs(ref))
    return _mel_close(got, ref)


def _forward_input(fam, batch, n_frames):
    n = G.n_samples(n_frames, fam.hop)
    if fam.dtype == "float64":
        return O.config_input(batch, n=n).astype(np.float64)
    return O.config_input(batch, n=n)


def _forward_points(fam):
    pts = G.forward_points(fam.fpb)
    if fam.name.startswith("mel-pc"):
        pts = pts + [p for p in G.PC_TILE_PHASE_PAIRS + G.PC_PRODUCER_PAIRS if p not in pts]
    return pts


@pytest.mark.parametrize("name", [f.name for f in G.FORWARD])
def test_forward_result_does_not_depend_on_iters(L, name):
    import torch

    fam = G.FORWARD_BY_NAME[name]
    ctx = L.get_context(0)
    ran = 0
    with _options(ctx, **fam.opts):
        for n_frames, iters_list in _group(_forward_points(fam)):
            y = _forward_input(fam, 3, n_frames)
            yt = torch.from_numpy(y).to("cuda:0")
            ctx.set_option("stft_iters", 0)
            base = _forward_call(L, fam, yt)
            assert base.shape[-1] == n_frames and _no_nan(base), (name, n_frames)
            assert _forward_close(fam, base.cpu().numpy(), _forward_oracle(fam, y)), (name, n_frames)
            for i in range(3):
                assert torch.equal(_forward_call(L, fam, yt[i]), base[i]), (name, n_frames, "clip alone", i)
            for iters in iters_list:
                ctx.set_option("stft_iters", iters)
                got = _forward_call(L, fam, yt)
                assert _no_nan(got), (name, n_frames, iters)
                assert torch.equal(got, base), (name, n_frames, iters)
                ran += 1
    print(f"{name}: {ran} geometry points, all bit-equal to the default result")


@pytest.mark.parametrize("name", G.EDGE_FORWARD)
def test_forward_grid_edge(L, name):
    """One workgroup per clip, so the grid is the batch: 63 (the last unmapped grid), 64 (the first mapped one), 65 and 71 (padded by 7 and
    by 1), 72; with and without the workgroup -> work item map."""
    import torch

    fam = G.FORWARD_BY_NAME[name]
    ctx = L.get_context(0)
    ran = 0
    with _options(ctx, **fam.opts):
        for batch in G.edge_batches_forward():
            assert G.forward_grid(batch, G.EDGE_ITERS, G.EDGE_ITERS, fam.fpb) == batch
            y = _forward_input(fam, batch, G.EDGE_ITERS)
            yt = torch.from_numpy(y).to("cuda:0")
            ctx.set_option("stft_iters", 0)
            ctx.set_option("xcd_remap", 1)
            base = _forward_call(L, fam, yt)
            assert base.shape[-1] == G.EDGE_ITERS and _no_nan(base), (name, batch)
            assert _forward_close(fam, base.cpu().numpy(), _forward_oracle(fam, y)), (name, batch)
            for i in (0, 31, batch - 8, batch - 1):
                assert torch.equal(_forward_call(L, fam, yt[i]), base[i]), (name, batch, "clip alone", i)
            for remap in (0, 1):
                ctx.set_option("xcd_remap", remap)
                for iters in (0, G.EDGE_ITERS):
                    ctx.set_option("stft_iters", iters)
                    got = _forward_call(L, fam, yt)
                    assert _no_nan(got), (name, batch, remap, iters)
                    assert torch.equal(got, base), (name, batch, remap, iters)
                    ran += 1
    print(f"{name}: {ran} grid-edge points, all bit-equal to the default result")


@pytest.mark.parametrize("name", G.ROUNDS_FORWARD)
def test_forward_more_than_one_round(L, name):
    """One frame per slot and enough short clips that the grid is at least three times the workgroups the device can hold at once."""
    import torch

    fam = G.FORWARD_BY_NAME[name]
    ctx = L.get_context(0)
    n_cu = _n_cu()
    batch = G.rounds_batch(n_cu, fam.fpb)
    assert G.forward_grid(batch, G.ROUNDS_FRAMES, 1, fam.fpb) >= 3 * n_cu * G.WAVE_SLOTS_PER_CU
    assert batch * G.ROUNDS_FRAMES < 65536, "below the size at which the library times its tuning variants (lra_api.hip [sel:autotune])"
    y = _forward_input(fam, batch, G.ROUNDS_FRAMES)
    yt = torch.from_numpy(y).to("cuda:0")
    with _options(ctx, **fam.opts):
        base = _forward_call(L, fam, yt)
        assert base.shape[-1] == G.ROUNDS_FRAMES and _no_nan(base)
        sample = (0, 1, batch // 3, batch - 2, batch - 1)
        for i in sample:
            assert _forward_close(fam, base[i].cpu().numpy(), _forward_oracle(fam, y[i])), (name, i)
            assert torch.equal(_forward_call(L, fam, yt[i]), base[i]), (name, "clip alone", i)
        for remap in (1, 0):
            ctx.set_option("xcd_remap", remap)
            ctx.set_option("stft_iters", 1)
            got = _forward_call(L, fam, yt)
            assert _no_nan(got), (name, remap)
            assert torch.equal(got, base), (name, remap)
            del got


def test_fused_mel_auto_rule_more_than_one_round(L):
    """stft_iters = 0: 5 * CU count + 3 clips of 9 000 samples are one workgroup per clip, 1.25 rounds of the producer / consumer kernel's four
    resident workgroups per CU -- the smallest form of the many-clip shape VERDICT.md asks for."""
    import torch

    fam = G.FORWARD_BY_NAME["mel-pc-hd4-p2-128"]
    ctx = L.get_context(0)
    batch = G.auto_rule_batch(_n_cu())
    y = O.config_input(batch, n=G.AUTO_RULE_SAMPLES)
    yt = torch.from_numpy(y).to("cuda:0")
    with _options(ctx):
        base = _forward_call(L, fam, yt)
        assert _no_nan(base)
        for i in (0, 1, batch // 2, 4 * _n_cu() - 1, 4 * _n_cu(), batch - 1):
            assert _forward_close(fam, base[i].cpu().numpy(), _forward_oracle(fam, y[i])), i
            assert torch.equal(_forward_call(L, fam, yt[i]), base[i]), ("clip alone", i)
        for iters in (3, 9):
            ctx.set_option("stft_iters", iters)
            assert torch.equal(_forward_call(L, fam, yt), base), iters
        ctx.set_option("stft_iters", 0)
        ctx.set_option("mel_pc", 0)  # the one-wave kernel on the same batch: rounding-level agreement (test_producer_consumer_mel_kernel's bar)
        one = _forward_call(L, fam, yt)
        assert bool(((base - one).abs() <= 2e-5 * one.abs()).all())


# ---- inverse ------------------------------------------------------------------------------------------------------------------------
def _inverse_case(fam, batch, n_used, use_length, seed):
    """(D as the oracle's spectrogram of a seeded signal, length, the oracle's inverse, its window envelope)."""
    rt = np.dtype(fam.dtype)
    n = G.n_samples(n_used, fam.hop)
    y = _signal(batch, n, rt, seed)
    D = O.stft(y, n_fft=fam.n_fft, hop_length=fam.hop)
    assert D.shape[-1] == n_used
    length = n if use_length else None  # (`length`: the clip's own length, which cuts the last hop block; without it the frames' whole reach)
    ref = O.istft(D, hop_length=fam.hop, n_fft=fam.n_fft, length=length)
    wss = _wss_for(dict(n_fft=fam.n_fft, hop_length=fam.hop), n_used, ref.shape[-1], length, rt)
    return D, length, ref, wss


def _inverse_call(L, fam, Dt, length):
    return L.istft(Dt, hop_length=fam.hop, n_fft=fam.n_fft, length=length)


@pytest.mark.parametrize("use_length", [False, True])
@pytest.mark.parametrize("name", [f.name for f in G.INVERSE])
def test_inverse_result_does_not_depend_on_strips(L, name, use_length):
    import torch

    fam = G.INVERSE_BY_NAME[name]
    ctx = L.get_context(0)
    ran = 0
    with _options(ctx, **fam.opts):
        for (n_used, batch), strips_list in _group([((nu, b), sf) for nu, sf, b in G.inverse_points(fam.fpb)]):
            D, length, ref, wss = _inverse_case(fam, batch, n_used, use_length, 100 * n_used + fam.hop)
            Dt = torch.from_numpy(D).to("cuda:0")
            ctx.set_option("istft_strip_groups", 0)
            base = _inverse_call(L, fam, Dt, length)
            assert _no_nan(base), (name, n_used)
            got = base.cpu().numpy()
            assert got.shape == ref.shape and got.dtype == ref.dtype
            assert _istft_close(got, ref, wss), (name, n_used)
            for i in range(batch):
                assert torch.equal(_inverse_call(L, fam, Dt[i], length), base[i]), (name, n_used, "clip alone", i)
            for strips in strips_list:
                ctx.set_option("istft_strip_groups", strips)
                got = _inverse_call(L, fam, Dt, length)
                assert _no_nan(got), (name, n_used, strips)
                assert torch.equal(got, base), (name, n_used, strips)
                ran += 1
    print(f"{name} length={use_length}: {ran} geometry points, all bit-equal to the default result")


@pytest.mark.parametrize("name", G.EDGE_INVERSE)
def test_inverse_grid_edge(L, name):
    """One strip per clip, FPB strips per workgroup: batches whose grids are 63, 64, 65, 71 and 72, with and without the map."""
    import torch

    fam = G.INVERSE_BY_NAME[name]
    ctx = L.get_context(0)
    ran = 0
    with _options(ctx, **fam.opts):
        for grid, batch in zip(G.EDGE_GRIDS, G.edge_batches_inverse(fam.fpb)):
            assert G.inverse_grid(batch, G.EDGE_STRIPS, G.EDGE_STRIPS, fam.fpb) == grid
            D, length, ref, wss = _inverse_case(fam, batch, G.EDGE_STRIPS, grid % 2 == 1, grid)
            Dt = torch.from_numpy(D).to("cuda:0")
            ctx.set_option("istft_strip_groups", 0)
            ctx.set_option("xcd_remap", 1)
            base = _inverse_call(L, fam, Dt, length)
            assert _no_nan(base), (name, batch)
            assert _istft_close(base.cpu().numpy(), ref, wss), (name, batch)
            for i in (0, batch // 2, batch - 2, batch - 1):
                assert torch.equal(_inverse_call(L, fam, Dt[i], length), base[i]), (name, batch, "clip alone", i)
            for remap in (0, 1):
                ctx.set_option("xcd_remap", remap)
                for strips in (0, G.EDGE_STRIPS):
                    ctx.set_option("istft_strip_groups", strips)
                    got = _inverse_call(L, fam, Dt, length)
                    assert _no_nan(got), (name, batch, remap, strips)
                    assert torch.equal(got, base), (name, batch, remap, strips)
                    ran += 1
    print(f"{name}: {ran} grid-edge points, all bit-equal to the default result")


@pytest.mark.parametrize("name", G.ROUNDS_INVERSE)
def test_inverse_more_than_one_round(L, name):
    """One frame per strip and enough short clips that the grid is at least three times the workgroups the device can hold at once."""
    import torch

    fam = G.INVERSE_BY_NAME[name]
    ctx = L.get_context(0)
    n_cu = _n_cu()
    batch = G.rounds_batch(n_cu, fam.fpb, inverse=True)
    assert G.inverse_grid(batch, G.ROUNDS_FRAMES, 1, fam.fpb) >= 3 * n_cu * G.WAVE_SLOTS_PER_CU
    n = G.n_samples(G.ROUNDS_FRAMES, fam.hop)
    y = _signal(batch, n, fam.dtype, 4048)
    with _options(ctx, **fam.opts):
        Dt = L.stft(torch.from_numpy(y).to("cuda:0"), n_fft=fam.n_fft, hop_length=fam.hop)  # (the spectrogram is made on the device: the oracle would take a minute)
        assert Dt.shape[-1] == G.ROUNDS_FRAMES
        base = _inverse_call(L, fam, Dt, n)
        assert _no_nan(base)
        wss = _wss_for(dict(n_fft=fam.n_fft, hop_length=fam.hop), G.ROUNDS_FRAMES, n, n, np.dtype(fam.dtype))
        for i in (0, 1, batch // 3, batch - 2, batch - 1):
            ref = O.istft(Dt[i].cpu().numpy(), hop_length=fam.hop, n_fft=fam.n_fft, length=n)
            assert _istft_close(base[i].cpu().numpy(), ref, wss), (name, i)
            assert torch.equal(_inverse_call(L, fam, Dt[i], n), base[i]), (name, "clip alone", i)
        for remap in (1, 0):
            ctx.set_option("xcd_remap", remap)
            ctx.set_option("istft_strip_groups", 1)
            got = _inverse_call(L, fam, Dt, n)
            assert _no_nan(got), (name, remap)
            assert torch.equal(got, base), (name, remap)
            del got
