"""GPU parity tests (run with ``-m gpu`` on the MI355X box): the HIP path, called through the C ABI by
the Python drop-in, against (1) the committed reference outputs in tests/golden/, (2) the CPU oracle
on seeded inputs, (3) size-independent properties at BASELINE.json's full sizes.

Tolerances (float32 pipeline vs the reference's float64-FFT-rounded-to-complex64):
  STFT   |d| <= 1e-5 |ref| + 2e-6 max|ref|        (observed ~2e-7 max|ref|)
  mel    |d| <= 1e-4 |ref| + 1e-4 max|ref|        (north-star bar; observed ~1e-6)
  ISTFT  |d| <= 4e-6 max|ref| / sqrt(wss) where the window sum-square is well conditioned; SNR >= 60 dB
  float64 pipeline: 1e-12 relative.
"""
import os
import warnings

import numpy as np
import pytest

import golden_cases
import stft_oracle as O

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

warnings.filterwarnings("ignore", message="n_fft=.*is too large")


@pytest.fixture(scope="module")
def L():
    import librosa_amd

    assert librosa_amd.device_count() > 0, "no HIP device: the product has no CPU fallback"
    return librosa_amd


def _stft_close(D, ref):
    scale = np.abs(ref).max()
    if D.dtype == np.complex128:
        return np.all(np.abs(D - ref) <= 1e-12 * scale)
    return np.all(np.abs(D - ref) <= 1e-5 * np.abs(ref) + 2e-6 * scale)


def _mel_close(M, ref):
    if M.dtype == np.float64:
        return np.all(np.abs(M - ref) <= 1e-11 * ref.max())
    return np.all(np.abs(M - ref) <= 1e-4 * np.abs(ref) + 1e-4 * ref.max())


def _istft_close(y, ref, wss):
    eps = 1e-12 if y.dtype == np.float64 else 4e-6
    cond = 1.0 / np.sqrt(np.maximum(wss.astype(np.float64), np.finfo(np.float32).tiny))
    tol = eps * np.abs(ref).max() * np.maximum(1.0, cond)
    well = wss > 1e-3 * wss.max()
    return np.all(np.abs(y - ref)[..., well] <= tol[well]) and np.all(np.abs(y - ref)[..., ~well] <= 50 * tol[~well] + 1e-3)


def _wss_for(skw, n_total_frames, out_len, length, dtype):
    n_fft = skw["n_fft"]
    win_length = skw.get("win_length")
    hop = skw.get("hop_length") or (win_length or n_fft) // 4
    center = skw.get("center", True)
    if length:
        padded = length + 2 * (n_fft // 2) if center else length
        n_frames = min(n_total_frames, int(np.ceil(padded / hop)))
    else:
        n_frames = n_total_frames
    wss = O.window_sumsquare(window=skw.get("window", "hann"), n_frames=n_frames, win_length=win_length, n_fft=n_fft, hop_length=hop, dtype=dtype)
    return O.fix_length(wss[(n_fft // 2 if center else 0) :], size=out_len)


@pytest.mark.parametrize("n_fft,hop", [(16384, 4096), (16384, 1000), (8192, 3000), (32, 8), (32, 5), (64, 32), (4096, 2048)])
def test_extreme_sizes(L, n_fft, hop):
    """Smallest and largest fused sizes, aligned and unaligned hops (n_fft = 16384 with a general hop does not fit the
    inverse kernel's LDS budget and must fall back to the rocFFT path transparently)."""
    rng = np.random.default_rng(n_fft + hop)
    y = rng.standard_normal((2, 70000)).astype(np.float32)
    D = L.stft(y, n_fft=n_fft, hop_length=hop)
    ref = O.stft(y, n_fft=n_fft, hop_length=hop)
    assert _stft_close(D, ref)
    yy = L.istft(D, hop_length=hop, length=y.shape[-1])
    assert np.abs(yy - O.istft(ref, hop_length=hop, length=y.shape[-1])).max() <= 2e-5
    if n_fft >= 512:
        M = L.feature.melspectrogram(y=y, n_fft=n_fft, hop_length=hop, n_mels=32)
        assert _mel_close(M, O.melspectrogram(y=y, n_fft=n_fft, hop_length=hop, n_mels=32))


def _sweep_seeds():
    """1, 2, 3 in the suite; LRA_SWEEP_SEEDS="4-40" (a range or a comma list) widens the sweep for a one-off stress run."""
    extra = os.environ.get("LRA_SWEEP_SEEDS", "")
    seeds = [1, 2, 3]
    for part in filter(None, extra.split(",")):
        lo, _, hi = part.partition("-")
        seeds += list(range(int(lo), int(hi or lo) + 1))
    return seeds


@pytest.mark.parametrize("seed", _sweep_seeds())
def test_random_configurations(L, seed):
    """Seeded sweep over (n_fft power of two or not, hop aligned or not or beyond n_fft, dtype, center, pad mode,
    win_length, 1-D / 2-D input): stft, istft and melspectrogram against the oracle.  The inverse is compared where
    the window sum-square is well conditioned with the golden cases' tolerance (`_istft_close`): y = acc / wss amplifies
    rounding noise by 1 / wss in the reference as much as here."""
    import warnings

    rng = np.random.default_rng(seed)
    bad = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(24):
            n_fft = int(rng.choice([64, 128, 256, 400, 512, 1000, 1024, 2048, 2049, 4096, 8192]))
            hop = int(rng.choice([max(1, n_fft // 8), n_fft // 4, n_fft // 2, n_fft // 3, n_fft, 160, 100, 441]))
            dtype = np.float64 if rng.random() < 0.25 else np.float32
            center = bool(rng.random() < 0.8)
            pad_mode = str(rng.choice(["constant", "reflect", "edge", "symmetric"]))
            n = int(rng.integers(max(n_fft, 2 * hop) + 3, 6 * n_fft + 4000))
            shape = (2, n) if rng.random() < 0.7 else (n,)
            win_length = None if rng.random() < 0.7 else int(n_fft * 3 // 4)
            y = rng.standard_normal(shape).astype(dtype)
            kw = dict(n_fft=n_fft, hop_length=hop, center=center, pad_mode=pad_mode, win_length=win_length)
            tag = (n_fft, hop, np.dtype(dtype).name, center, pad_mode, n, win_length, shape)
            f32 = dtype == np.float32
            D, ref = L.stft(y, **kw), O.stft(y, **kw)
            if not np.abs(D - ref).max() <= (4e-6 if f32 else 1e-12) * np.abs(ref).max():
                bad.append(("stft",) + tag)
            ikw = dict(hop_length=hop, center=center, win_length=win_length, n_fft=n_fft)
            try:
                yr = O.istft(ref, **ikw)
            except Exception:
                yr = None  # the reference rejects this combination (e.g. no frame fits): nothing to compare
            if yr is not None:
                yy = L.istft(D, **ikw)
                wss = O.window_sumsquare(window="hann", n_frames=ref.shape[-1], win_length=win_length, n_fft=n_fft, hop_length=hop, dtype=np.float64)
                wss = wss[(n_fft // 2 if center else 0):]
                wss = np.pad(wss, (0, max(0, yr.shape[-1] - len(wss))))[: yr.shape[-1]]
                # the golden cases' bar: 4e-6 max|ref| scaled by the conditioning 1 / sqrt(wss) of the division (core/spectrum.py:622-624)
                if yy.shape != yr.shape or not _istft_close(yy, yr, wss.astype(yr.dtype)):
                    bad.append(("istft",) + tag + (float(np.abs(yy - yr).max() / max(np.abs(yr).max(), 1e-30)),))
            if n_fft >= 256:
                mk = dict(kw, n_mels=int(rng.choice([20, 40, 64, 128])), power=float(rng.choice([1.0, 2.0, 1.5])))
                M, Mr = L.feature.melspectrogram(y=y, **mk), O.melspectrogram(y=y, **mk)
                if not np.abs(M - Mr).max() <= (2e-5 if f32 else 1e-11) * Mr.max():
                    bad.append(("mel",) + tag)
    assert not bad, bad


@pytest.mark.parametrize("seed", [s + 100 for s in _sweep_seeds()] + [110, 111, 112, 113, 114])
def test_random_configurations_wide(L, seed):
    """The argument space around the first sweep (the generator of tests/test_oracle.py::test_oracle_vs_live_reference_wide, which pins the oracle on
    exactly these draws): named / tuple / array windows, win_length, symmetric padding, float64, 1-D to 3-D input, hops beyond the frame,
    mel scale / norm / band-edge options -- drop-in against oracle."""
    import warnings

    rng = np.random.default_rng(seed)
    n_fft = int(rng.choice([64, 200, 256, 512, 1000, 1024, 2048, 4096]))
    hop = int(rng.choice([n_fft // 4, n_fft // 2, n_fft // 3, n_fft, max(1, n_fft // 8), n_fft + 17]))
    dtype = np.float64 if rng.random() < 0.3 else np.float32
    center = bool(rng.random() < 0.7)
    pad_mode = str(rng.choice(["constant", "reflect", "edge", "symmetric"]))
    win_length = None if rng.random() < 0.6 else int(rng.integers(n_fft // 2, n_fft))
    wl = win_length or n_fft
    window = [lambda: "hann", lambda: "hamming", lambda: "blackmanharris", lambda: ("tukey", 0.25), lambda: ("kaiser", 4.0), lambda: rng.random(wl) + 0.1][int(rng.integers(0, 6))]()
    n = int(rng.integers(max(n_fft, 2 * hop) + 5, 5 * n_fft + 3000))
    shape = [(n,), (2, n), (2, 3, n)][int(rng.integers(0, 3))]
    y = rng.standard_normal(shape).astype(dtype)
    kw = dict(n_fft=n_fft, hop_length=hop, win_length=win_length, window=window, center=center, pad_mode=pad_mode)
    f32 = dtype == np.float32
    tag = (seed, n_fft, hop, np.dtype(dtype).name, center, pad_mode, win_length, str(window)[:20], shape)
    D, ref = L.stft(y, **kw), O.stft(y, **kw)
    assert D.dtype == ref.dtype and D.shape == ref.shape, tag
    assert np.abs(D - ref).max() <= (4e-6 if f32 else 1e-12) * np.abs(ref).max(), tag
    ikw = dict(hop_length=hop, win_length=win_length, n_fft=n_fft, window=window, center=center)
    try:
        yr = O.istft(ref, **ikw)
    except Exception:
        yr = None
    if yr is not None:
        yy = L.istft(D, **ikw)
        wss = O.window_sumsquare(window=window, n_frames=ref.shape[-1], win_length=win_length, n_fft=n_fft, hop_length=hop, dtype=np.float64)
        wss = wss[(n_fft // 2 if center else 0):]
        wss = np.pad(wss, (0, max(0, yr.shape[-1] - len(wss))))[: yr.shape[-1]]
        assert yy.shape == yr.shape and yy.dtype == yr.dtype, tag
        assert _istft_close(yy, yr, wss.astype(yr.dtype)), tag + (float(np.abs(yy - yr).max()),)
    if n_fft >= 200:
        mk = dict(kw, sr=22050, n_mels=int(rng.choice([13, 40, 80, 128])), power=float(rng.choice([1.0, 2.0, 1.5])), htk=bool(rng.random() < 0.3),
                  norm=[None, "slaney", 1, np.inf][int(rng.integers(0, 4))], fmin=float(rng.choice([0.0, 50.0])), fmax=[None, 8000.0][int(rng.integers(0, 2))])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            M, Mr = L.feature.melspectrogram(y=y, **mk), O.melspectrogram(y=y, **mk)
        assert M.dtype == Mr.dtype and M.shape == Mr.shape, tag
        assert np.abs(M - Mr).max() <= (2e-5 if f32 else 1e-11) * Mr.max(), tag


def test_threads_share_a_context(L):
    """Several Python threads calling the drop-in concurrently (ctypes releases the GIL): public calls serialise on a
    per-context lock, so stream selection, the sticky non-finite flag and plan scratch buffers cannot interleave."""
    import threading
    import warnings

    errs = []

    def work(seed):
        rng = np.random.default_rng(seed)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for it in range(8):
                n_fft = int(rng.choice([400, 512, 1024, 2048]))
                hop = n_fft // 4
                y = rng.standard_normal((3, int(rng.integers(6000, 30000)))).astype(np.float32)
                try:
                    D = L.stft(y, n_fft=n_fft, hop_length=hop)
                    if not _stft_close(D, O.stft(y, n_fft=n_fft, hop_length=hop)):
                        errs.append(("stft", seed, it))
                    M = L.feature.melspectrogram(y=y, n_fft=n_fft, hop_length=hop, n_mels=64)
                    if not _mel_close(M, O.melspectrogram(y=y, n_fft=n_fft, hop_length=hop, n_mels=64)):
                        errs.append(("mel", seed, it))
                    if not np.abs(L.istft(D, hop_length=hop, length=y.shape[-1]) - y).max() <= 2e-5:
                        errs.append(("istft", seed, it))
                except Exception as exc:  # noqa: BLE001 -- collected and reported by the main thread
                    errs.append(("exception", seed, it, repr(exc)[:120]))

    threads = [threading.Thread(target=work, args=(s,)) for s in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs[:5]


def test_mel_epilogue_forms_agree(L):
    """The run-ordered two-slope epilogue (default where it applies), the masked two-slope fallback and the generic
    banded path must all match the oracle: 128 / 80 mels (run-ordered), 40 mels (too many pieces: falls back)."""
    import torch

    yh = O.config_input(3, n=30000)
    y = torch.from_numpy(yh).cuda()
    ctx = L.get_context(0)
    bad = []
    try:
        for n_fft, hop, n_mels, power in ((2048, 512, 128, 2.0), (2048, 512, 80, 1.0), (2048, 256, 40, 2.0), (1024, 256, 80, 2.0), (1024, 256, 64, 1.5)):
            Mref = O.melspectrogram(y=yh, n_fft=n_fft, hop_length=hop, n_mels=n_mels, power=power)
            for runs, generic in ((1, 0), (0, 0), (0, 1)):
                ctx.set_option("mel_runs", runs)
                ctx.set_option("generic_mel", generic)
                M = L.feature.melspectrogram(y=y, n_fft=n_fft, hop_length=hop, n_mels=n_mels, power=power).cpu().numpy()
                if not _mel_close(M, Mref):
                    bad.append((n_fft, hop, n_mels, power, runs, generic, float(np.abs(M - Mref).max() / Mref.max())))
    finally:
        ctx.set_option("mel_runs", 1)
        ctx.set_option("generic_mel", 0)
    assert not bad, bad


def test_autotune_picks_a_variant_and_stays_correct(L):
    """A large first call times the kernel variants on its own buffers; the result must be unaffected."""
    import torch

    yh = O.config_input(130, n=22050 * 12)  # 130 x 517 = 67 210 frames: above the autotune threshold (65 536)
    y = torch.from_numpy(yh).cuda()
    ctx = L.get_context(0)
    window = np.asarray(L.filters.get_window("hann", 2048, fftbins=True), dtype=np.float32)
    ctx.set_option("autotune", 1)
    D = L.stft(y, n_fft=2048, hop_length=512)
    M = L.feature.melspectrogram(y=y, n_fft=2048, hop_length=512)
    yy = L.istft(D, hop_length=512, length=yh.shape[-1])
    torch.cuda.synchronize()
    plan = ctx.stft_plan(2048, 512, window, True, "constant", np.float32)
    # (the complex-out epilogue runs the second-generation kernel, which has no variants: nothing to tune there)
    assert ctx.tuned_variant(plan, 0) == -1 and ctx.tuned_variant(plan, 2) in (0, 4)
    k = 5  # spot-check a clip against the oracle
    assert _stft_close(D[k].cpu().numpy(), O.stft(yh[k], n_fft=2048, hop_length=512))
    assert _mel_close(M[k].cpu().numpy(), O.melspectrogram(y=yh[k], n_fft=2048, hop_length=512))
    assert np.abs(yy[k].cpu().numpy() - yh[k]).max() <= 2e-5


# ---------------------------------------------------------------------------------------------------
# 1. committed reference outputs
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(golden_cases.CASES))
def test_golden_case(L, name):
    case = golden_cases.CASES[name]
    g = np.load(os.path.join(GOLDEN_DIR, f"{name}.npz"))
    y = g["y"]
    skw = dict(case["stft"])
    D = L.stft(y, **skw)
    assert D.shape == g["D"].shape and D.dtype == g["D"].dtype
    assert _stft_close(D, g["D"])
    if case["mel"] is not None:
        power, fkw = golden_cases.split_mel_kwargs(case["mel"])
        mkw = dict(skw)
        mkw.setdefault("hop_length", int(skw.get("win_length", skw["n_fft"]) // 4))
        M = L.feature.melspectrogram(y=y, sr=golden_cases.SR, power=power, **mkw, **fkw)
        assert M.shape == g["mel"].shape and M.dtype == g["mel"].dtype
        assert _mel_close(M, g["mel"])
        assert np.array_equal(L.filters.mel(sr=golden_cases.SR, n_fft=skw["n_fft"], **fkw), g["mel_basis"])
        # melspectrogram(S=...) with the reference's power spectrogram as input
        S = np.abs(g["D"]) ** power
        M2 = L.feature.melspectrogram(S=S, sr=golden_cases.SR, **fkw)
        assert _mel_close(M2, g["mel"])
        # _spectrogram
        S3, nf = L._spectrogram(y=y, power=power, **mkw)
        assert nf == skw["n_fft"] and S3.shape == S.shape
        assert np.all(np.abs(S3 - S) <= 1e-4 * np.abs(S) + 1e-5 * S.max())
    if case["istft"]:
        ikw = {k: v for k, v in skw.items() if k in ("hop_length", "win_length", "n_fft", "window", "center")}
        for key, length in (("y_istft_len", y.shape[-1]), ("y_istft_nolen", None)):
            ref = g[key]
            yh = L.istft(g["D"], length=length, **ikw)
            assert yh.shape == ref.shape and yh.dtype == ref.dtype
            wss = _wss_for(skw, g["D"].shape[-1], ref.shape[-1], length, ref.dtype)
            assert _istft_close(yh, ref, wss), (name, key)


def test_golden_config1(L):
    g = np.load(os.path.join(GOLDEN_DIR, "config1_sine10s.npz"))
    y = O.config1_input()
    D = L.stft(y, n_fft=2048, hop_length=512)
    assert D.shape == (1025, 431) and D.dtype == np.complex64
    # pure tone: element-wise relative error is meaningless below f32's leakage floor
    assert np.abs(D[:, g["frames"]] - g["D_frames"]).max() <= 2e-6 * g["D_absmax"]
    M = L.feature.melspectrogram(y=y, sr=22050, n_fft=2048, hop_length=512, n_mels=128)
    assert np.all(np.abs(M - g["mel"]) <= 1e-4 * np.abs(g["mel"]) + 1e-4 * g["mel"].max())
    yh = L.istft(D, hop_length=512, length=len(y))
    assert np.abs(yh[:4096] - g["y_istft_head"]).max() <= 4e-6 and np.abs(yh[-4096:] - g["y_istft_tail"]).max() <= 4e-6
    snr = 10 * np.log10(np.sum(y.astype(np.float64) ** 2) / np.sum((y - yh).astype(np.float64) ** 2))
    assert snr >= 60


def test_golden_config2_clips(L):
    g = np.load(os.path.join(GOLDEN_DIR, "config2_clips.npz"))
    Y = np.stack([O.config_input(1, first_clip=i)[0] for i in (0, 37)])
    D = L.stft(Y, n_fft=2048, hop_length=512)
    M = L.feature.melspectrogram(y=Y, sr=22050, n_fft=2048, hop_length=512, n_mels=128)
    assert D.shape == (2, 1025, 1292) and M.shape == (2, 128, 1292)
    for j, i in enumerate((0, 37)):
        assert np.abs(D[j][:, g["frames"]] - g[f"D_frames_{i}"]).max() <= 2e-6 * g[f"D_absmax_{i}"]
    assert _mel_close(M[0], g["mel_0"])
    ref37 = g["mel_frames_37"]
    assert np.all(np.abs(M[1][:, g["frames"]] - ref37) <= 1e-4 * np.abs(ref37) + 1e-4 * g["mel_absmax_37"])
    # the north star's own wording, "mel within 1e-4 rel": on this noise-floored input every band is well above zero, so
    # the PURE relative error is meaningful -- no max() term to hide behind (observed ~5e-6)
    assert np.all(np.abs(M[0] - g["mel_0"]) <= 1e-4 * np.abs(g["mel_0"]))
    assert np.all(np.abs(M[1][:, g["frames"]] - ref37) <= 1e-4 * np.abs(ref37))


# ---------------------------------------------------------------------------------------------------
# 2. oracle on seeded inputs (reference test parametrisations: tests/test_core.py:256-371, 813-828)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", [256, 501, 1023, 2048])
@pytest.mark.parametrize("hop", [None, 128, 129])
@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("window", ["hann", "ones"])
def test_stft_vs_oracle(L, n_fft, hop, center, window):
    y = golden_cases.make_signal("chirp", 8192, 0) + golden_cases.make_signal("noise", 8192, n_fft) * 0.1
    D = L.stft(y, n_fft=n_fft, hop_length=hop, center=center, window=window)
    ref = O.stft(y, n_fft=n_fft, hop_length=hop, center=center, window=window)
    assert D.shape == ref.shape and D.dtype == ref.dtype
    assert _stft_close(D, ref)


@pytest.mark.parametrize("n_fft", [1024, 1025, 2048, 4096])
@pytest.mark.parametrize("hop", [128, 256, 512])
@pytest.mark.parametrize("window", ["hann", "blackmanharris"])
def test_istft_reconstruction(L, n_fft, hop, window):
    # tests/test_core.py:813-828 (reference): stft -> istft reproduces the signal
    x = golden_cases.make_signal("chirp", 22050, 0)
    D = L.stft(x, n_fft=n_fft, hop_length=hop, window=window)
    xh = L.istft(D, hop_length=hop, window=window, n_fft=n_fft, length=len(x))
    assert xh.shape == x.shape and np.isfinite(xh).all()
    assert np.abs(x - xh).max() <= 2e-5
    ref = O.istft(O.stft(x, n_fft=n_fft, hop_length=hop, window=window), hop_length=hop, window=window, n_fft=n_fft, length=len(x))
    assert np.abs(xh - ref).max() <= 2e-5


@pytest.mark.parametrize("pad_mode", ["constant", "reflect", "edge", "symmetric", "linear_ramp"])
def test_pad_modes(L, pad_mode):
    y = golden_cases.make_signal("noise", 3000, 5, (2,))
    D = L.stft(y, n_fft=512, hop_length=128, pad_mode=pad_mode)
    assert _stft_close(D, O.stft(y, n_fft=512, hop_length=128, pad_mode=pad_mode))


def test_multichannel_equals_per_channel(L):
    # tests/test_multichannel.py:96-111, 685-714: leading axes are independent
    y = golden_cases.make_signal("noise", 9000, 3, (2, 3))
    D = L.stft(y, n_fft=1024, hop_length=256)
    M = L.feature.melspectrogram(y=y, n_fft=1024, hop_length=256, n_mels=40)
    for i in range(2):
        for j in range(3):
            assert np.array_equal(D[i, j], L.stft(y[i, j], n_fft=1024, hop_length=256))
            assert np.array_equal(M[i, j], L.feature.melspectrogram(y=y[i, j], n_fft=1024, hop_length=256, n_mels=40))
    yh = L.istft(D, hop_length=256, length=9000)
    assert np.array_equal(yh[1, 2], L.istft(D[1, 2], hop_length=256, length=9000))


def test_float64_path(L):
    y = golden_cases.make_signal("chirp", 16000, 1, None, "float64")
    D = L.stft(y, n_fft=2048, hop_length=512)
    ref = O.stft(y, n_fft=2048, hop_length=512)
    assert D.dtype == np.complex128 and _stft_close(D, ref)
    yh = L.istft(D, hop_length=512, length=len(y))
    assert yh.dtype == np.float64 and np.abs(yh - y).max() < 1e-12
    M = L.feature.melspectrogram(y=y, n_fft=2048, hop_length=512)
    assert M.dtype == np.float64 and _mel_close(M, O.melspectrogram(y=y, n_fft=2048, hop_length=512))
    # dtype= overrides: f32 audio -> complex128 result is the exact-mode transform of the f32 samples
    y32 = y.astype(np.float32)
    D2 = L.stft(y32, n_fft=2048, hop_length=512, dtype=np.complex128)
    assert D2.dtype == np.complex128 and _stft_close(D2, O.stft(y32, n_fft=2048, hop_length=512, dtype=np.complex128))


def test_out_parameter(L):
    # tests/test_core.py:317-371, 2941-2963 (reference)
    y = golden_cases.make_signal("noise", 8192, 2, (2,))
    D = L.stft(y, n_fft=2048, hop_length=512)
    out = np.zeros_like(D, order="C")
    D2 = L.stft(y, n_fft=2048, hop_length=512, out=out)
    assert D2 is out and np.array_equal(D2, D)
    big = np.zeros(D.shape[:-1] + (D.shape[-1] + 5,), dtype=D.dtype)
    D3 = L.stft(y, n_fft=2048, hop_length=512, out=big)
    assert D3.shape == D.shape and np.array_equal(D3, D) and np.shares_memory(D3, big)
    with pytest.raises(L.ParameterError):
        L.stft(y, n_fft=2048, hop_length=512, out=np.zeros(D.shape[:-1] + (D.shape[-1] - 1,), dtype=D.dtype))
    with pytest.raises(L.ParameterError):
        L.stft(y, n_fft=2048, hop_length=512, out=np.zeros(D.shape, dtype=np.float32))
    yo = np.ones((2, 8192), dtype=np.float32)
    y2 = L.istft(D, hop_length=512, length=8192, out=yo)
    assert y2 is yo and np.abs(y2 - y).max() < 2e-5
    with pytest.raises(L.ParameterError):
        L.istft(D, hop_length=512, length=8192, out=np.zeros((2, 8000), dtype=np.float32))


def test_c_order_spectrogram_input(L):
    """istft / melspectrogram(S=) accept a C-ordered (bins, frames) array, as the reference does."""
    y = golden_cases.make_signal("mix", 22050, 4)
    D = np.ascontiguousarray(O.stft(y, n_fft=2048, hop_length=512))
    yh = L.istft(D, hop_length=512, length=len(y))
    assert np.abs(yh - y).max() < 2e-5
    S = np.ascontiguousarray(np.abs(D) ** 2)
    M = L.feature.melspectrogram(S=S, sr=22050)
    assert _mel_close(M, O.melspectrogram(S=S, sr=22050))


def test_errors_and_warnings(L):
    y = np.zeros(1000, dtype=np.float32)
    with pytest.raises(L.ParameterError):
        L.stft(y, n_fft=2048, center=False)
    with pytest.warns(UserWarning):
        D = L.stft(y, n_fft=2048)
    assert D.shape == (1025, 2)  # 1 + 1000 // 512
    with pytest.raises(L.ParameterError):
        L.stft(y, n_fft=512, pad_mode="wrap")
    with pytest.raises(L.ParameterError):
        L.stft(np.array([0.0, np.inf, 1.0] * 400, dtype=np.float32), n_fft=512)
    with pytest.raises(L.ParameterError):
        L.feature.melspectrogram(y=y, n_fft=512, norm="bogus")


# ---------------------------------------------------------------------------------------------------
# 3. device-resident (torch tensor) interface
# ---------------------------------------------------------------------------------------------------
def test_torch_device_tensors(L):
    import torch

    y = O.config_input(3, n=30000)
    yt = torch.from_numpy(y).cuda()
    D = L.stft(yt, n_fft=2048, hop_length=512)
    assert D.is_cuda and D.dtype == torch.complex64 and tuple(D.shape) == (3, 1025, 59)
    ref = O.stft(y, n_fft=2048, hop_length=512)
    assert _stft_close(D.cpu().numpy(), ref)
    M = L.feature.melspectrogram(y=yt, sr=22050, n_fft=2048, hop_length=512, n_mels=128)
    assert M.is_cuda and _mel_close(M.cpu().numpy(), O.melspectrogram(y=y, sr=22050, n_fft=2048, hop_length=512, n_mels=128))
    yh = L.istft(D, hop_length=512, length=30000)
    assert yh.is_cuda and np.abs(yh.cpu().numpy() - y).max() < 2e-5
    # the in-kernel non-finite flag replaces valid_audio's host scan for device tensors
    bad = yt.clone()
    bad[1, 12345] = float("nan")
    with pytest.raises(L.ParameterError):
        L.stft(bad, n_fft=2048, hop_length=512)
    with pytest.raises(L.ParameterError):
        L.feature.melspectrogram(y=bad, n_fft=2048, hop_length=512)
    L.stft(bad, n_fft=2048, hop_length=512, check_finite=False)  # opt-out does not raise
    with pytest.raises(L.ParameterError):
        L.stft(bad, n_fft=1023, hop_length=512)  # general (rocFFT) path: explicit device scan


@pytest.mark.parametrize("name", ["stft_n2048_h512_1s", "stft_n1024_blackmanharris", "stft_n4096_h512", "stft_stereo_n1024", "stft_f64_n2048", "stft_n512_reflect"])
def test_padded_row_view_against_goldens(L, name, monkeypatch):
    """Round 5 (optional layout, LRA_ROW_ALIGN / row_align=128): a device-resident stft result with each frame's row on a 128-byte boundary
    behind the (..., n_bins, n_frames) view (core/spectrum.py:356 allocates a strided view too).  Strides as documented, values = the
    reference's golden, bit-equal to the packed form, nothing written into the padding, istft / _spectrogram / the other consumers take
    the view as it is."""
    import torch

    from librosa_amd.core import spectrum as SP

    case = golden_cases.CASES[name]
    g = np.load(os.path.join(GOLDEN_DIR, f"{name}.npz"))
    skw = dict(case["stft"])
    n_fft = skw["n_fft"]
    n_bins = 1 + n_fft // 2
    y = g["y"]
    yt = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    csize = 16 if y.dtype == np.float64 else 8
    assert L.stft(yt, **skw).stride(-1) == (n_bins if SP.ROW_ALIGN_BYTES == 0 else SP.row_pitch(n_bins, csize))  # the default: packed rows
    monkeypatch.setattr(SP, "ROW_ALIGN_BYTES", 128)        # the module-wide switch (env LRA_ROW_ALIGN); row_align= overrides it per call
    monkeypatch.setattr(SP._arrays, "POISON_OUTPUTS", True)  # results start as NaN bit patterns: whatever the kernels leave alone stays NaN
    D = L.stft(yt, **skw)
    Dp = L.stft(yt, row_align=0, **skw)
    monkeypatch.setattr(SP._arrays, "POISON_OUTPUTS", False)
    pitch = SP.row_pitch(n_bins, csize)
    assert (pitch * csize) % 128 == 0 or pitch == n_bins
    assert (pitch > n_bins) == (n_bins * csize >= 4096)
    assert tuple(D.shape) == g["D"].shape == tuple(Dp.shape)
    assert D.stride(-2) == 1 and D.stride(-1) == pitch and Dp.stride(-1) == n_bins
    assert torch.equal(D, Dp)
    assert _stft_close(D.cpu().numpy(), g["D"])
    if pitch > n_bins:  # the padding behind the view is still the poison pattern
        assert D.data_ptr() % 128 == 0
        n_frames = D.shape[-1]
        base = torch.as_strided(D, (D.numel() // (n_bins * n_frames), n_frames, pitch), (n_frames * pitch, pitch, 1))
        assert bool(torch.isnan(torch.view_as_real(base[..., n_bins:])).all())
        assert not bool(torch.isnan(torch.view_as_real(base[..., :n_bins])).any())
    hop = skw.get("hop_length") or (skw.get("win_length") or n_fft) // 4
    ikw = {k: v for k, v in skw.items() if k in ("hop_length", "win_length", "n_fft", "window", "center")}
    ya, yb = L.istft(D, length=y.shape[-1], **ikw), L.istft(Dp, length=y.shape[-1], **ikw)
    assert torch.equal(ya, yb)
    assert torch.equal(L.istft(D.contiguous(), length=y.shape[-1], **ikw), ya)  # (a C-ordered copy goes through the transposing path)
    assert np.abs(ya.cpu().numpy() - y).max() < (1e-10 if y.dtype == np.float64 else 5e-5)
    S, _ = L._spectrogram(y=yt, power=2, **{**{k: v for k, v in skw.items() if k != "dtype"}, "hop_length": hop})
    assert S.stride(-2) == 1 and S.stride(-1) == SP.row_pitch(n_bins, csize // 2)
    P = np.abs(g["D"].astype(np.complex128)) ** 2
    assert np.all(np.abs(S.cpu().numpy() - P) <= 1e-4 * P + 1e-5 * P.max())
    mag, ph = L.magphase(D)
    mag2, ph2 = L.magphase(Dp)
    assert torch.equal(mag, mag2) and torch.equal(ph, ph2)
    M1 = L.feature.melspectrogram(S=S, sr=22050, n_mels=40)
    M2 = L.feature.melspectrogram(S=S.contiguous(), sr=22050, n_mels=40)
    assert torch.allclose(M1, M2, rtol=1e-5, atol=0)


def test_tuning_variants_agree(L):
    """The tuning variants of the n_fft=2048 kernels must agree with the oracle and each other."""
    import torch

    yh = O.config_input(2, n=44100)
    y = torch.from_numpy(yh).cuda()
    Dref = O.stft(yh, n_fft=2048, hop_length=512)
    Mref = O.melspectrogram(y=yh, n_fft=2048, hop_length=512)
    ctx = L.get_context(0)
    bad = []
    try:
        for v in (0, 1, 4):
            ctx.set_option("variant", v)
            for iters in (1, 3, 16):
                ctx.set_option("stft_iters", iters)
                D = L.stft(y, n_fft=2048, hop_length=512)
                M = L.feature.melspectrogram(y=y, n_fft=2048, hop_length=512).cpu().numpy()
                yy = L.istft(D, hop_length=512, length=44100).cpu().numpy()
                if not _stft_close(D.cpu().numpy(), Dref):
                    bad.append((v, iters, "stft", float(np.abs(D.cpu().numpy() - Dref).max())))
                if not _mel_close(M, Mref):
                    bad.append((v, iters, "mel", float(np.abs(M - Mref).max())))
                if not np.abs(yy - yh).max() <= 2e-5:
                    bad.append((v, iters, "istft", float(np.abs(yy - yh).max())))
    finally:
        ctx.set_option("variant", -1)
        ctx.set_option("stft_iters", 0)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------
# 4. BASELINE.json full sizes: size-independent properties (the oracle would take minutes here)
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_batch():
    import torch

    torch.manual_seed(440)
    B, n = 256, 661500
    t = torch.arange(n, device="cuda", dtype=torch.float32) / 22050.0
    f = 110.0 * 2.0 ** ((torch.arange(B, device="cuda") % 72).float() / 12.0)
    y = 0.1 * torch.randn(B, n, device="cuda") + 0.5 * torch.sin(2 * np.pi * f[:, None] * t[None, :])
    return y.clamp_(-1, 1).contiguous()


def test_full_size_mel_properties(L, full_batch):
    """config 2: batch=256 x 30 s.  Batch == per-clip; a sampled subset equals the oracle; linearity in
    power (scaling the audio by a scales mel by a^2)."""
    y = full_batch
    # batch == per clip is asserted bit for bit below: pin the kernel variant for it.  Left to the autotune, the first large call may keep
    # variant 4 for the batch while a single clip (too small to tune on) runs variant 0, and the two agree only to tolerance
    # (test_tuning_variants_agree); VERDICT r03.
    ctx = L.get_context(0)
    ctx.set_option("variant", 0)
    try:
        _full_size_mel_properties(L, y)
    finally:
        ctx.set_option("variant", -1)


def _full_size_mel_properties(L, y):
    M = L.feature.melspectrogram(y=y, sr=22050, n_fft=2048, hop_length=512, n_mels=128)
    assert tuple(M.shape) == (256, 128, 1292)
    Mh = M.cpu().numpy()
    assert np.isfinite(Mh).all() and (Mh >= 0).all()
    for i in (0, 1, 100, 255):
        yi = y[i].cpu().numpy()
        ref = O.melspectrogram(y=yi, sr=22050, n_fft=2048, hop_length=512, n_mels=128)
        assert _mel_close(Mh[i], ref), i
        assert np.all(np.abs(Mh[i] - ref) <= 1e-4 * np.abs(ref)), (i, (np.abs(Mh[i] - ref) / np.abs(ref)).max())  # pure relative, 1e-4
        assert np.array_equal(L.feature.melspectrogram(y=y[i], sr=22050, n_fft=2048, hop_length=512, n_mels=128).cpu().numpy(), Mh[i])
    M2 = L.feature.melspectrogram(y=2.0 * y[:32], sr=22050, n_fft=2048, hop_length=512, n_mels=128).cpu().numpy()
    assert np.allclose(M2, 4.0 * Mh[:32], rtol=1e-5, atol=0)


def test_full_size_stft_istft_round_trip(L, full_batch):
    """config 4: stft -> istft on batch=256 x 30 s, reconstruction SNR >= 60 dB for every clip; plus
    Parseval: sum_t sum_f c_f |D|^2 / n_fft == sum_t sum_n (w x)^2 per frame (checked via window power)."""
    y = full_batch
    D = L.stft(y, n_fft=2048, hop_length=512)
    assert tuple(D.shape) == (256, 1025, 1292)
    yh = L.istft(D, hop_length=512, length=y.shape[-1])
    err = (y - yh).double().pow(2).sum(dim=1)
    sig = y.double().pow(2).sum(dim=1)
    snr = 10 * np.log10((sig / err).cpu().numpy())
    assert snr.min() >= 60, snr.min()
    # a sampled clip against the oracle
    ref = O.stft(y[17].cpu().numpy(), n_fft=2048, hop_length=512)
    assert _stft_close(D[17].cpu().numpy(), ref)
    # Parseval on the Hermitian half-spectrum: energy of each windowed frame
    P = D.abs().double().pow(2)
    c = np.full(1025, 2.0)
    c[0] = c[-1] = 1.0
    import torch

    e_freq = (P * torch.from_numpy(c).cuda()[None, :, None]).sum(dim=1) / 2048.0  # (256, 1292)
    frames = y[:4].unfold(-1, 2048, 512)  # interior frames of 4 clips: t = 2 .. (centred offset of 2 frames)
    w = torch.from_numpy(O.get_window("hann", 2048).astype(np.float32)).cuda()
    e_time = (frames * w).double().pow(2).sum(dim=-1)  # (4, 1288)
    assert torch.allclose(e_freq[:4, 2 : 2 + e_time.shape[1]], e_time, rtol=1e-5)


def test_multi_resolution_stack(L, full_batch):
    """config 5 (CQT-lite): three STFTs at n_fft = 512 / 2048 / 8192 sharing hop = 512 share a time grid."""
    y = full_batch[:8]
    outs = [L.stft(y, n_fft=n, hop_length=512) for n in (512, 2048, 8192)]
    assert [tuple(o.shape) for o in outs] == [(8, 257, 1292), (8, 1025, 1292), (8, 4097, 1292)]
    yi = y[3].cpu().numpy()
    for n, o in zip((512, 2048, 8192), outs):
        assert _stft_close(o[3].cpu().numpy(), O.stft(yi, n_fft=n, hop_length=512))


@pytest.mark.parametrize("hop", [512, 1024, 2048, 4096, 8192])
def test_large_frame_ring_forms(L, hop):
    """n_fft = 8192 (four waves per frame) over every register-ring form and direct framing -- hop = n_fft / 16 and n_fft / 2 run the last pass
    mirrored across the halves of a wave (lra_kernels.h, mirror32_*), the others split through LDS -- complex, magnitude, power and general-power
    epilogues, odd lengths, two channels, reflect and zero padding, uncentred: against the oracle with the golden cases' bar."""
    rng = np.random.default_rng(8192 + hop)
    for n, center, pad_mode in ((70001, True, "reflect"), (41234, True, "constant"), (52345, False, "constant")):
        y = rng.standard_normal((2, n)).astype(np.float32)
        kw = dict(n_fft=8192, hop_length=hop, center=center, pad_mode=pad_mode)
        assert _stft_close(L.stft(y, **kw), O.stft(y, **kw)), (hop, n, center, pad_mode)
        for power in (1.0, 2.0, 1.5):
            S, _ = L.core.spectrum._spectrogram(y=y, power=power, **kw)
            Sr, _ = O.spectrogram(y=y, power=power, **kw)
            assert np.abs(S - Sr).max() <= 8e-6 * np.abs(Sr).max(), (hop, n, center, pad_mode, power)


@pytest.mark.parametrize("clips", [1, 2])
@pytest.mark.parametrize("hd", [1, 2, 4, 8])
def test_second_generation_kernel_n16384(L, hd, clips):
    """n_fft = 16384 with hop = n_fft / {1, 2, 4, 8}: the second-generation forward kernel (csrc/lra_fused.h, instance group 13) -- complex, magnitude,
    power and general-power epilogues on 3 n_fft + 1 samples, against the oracle with the bars of test_large_frame_ring_forms."""
    n_fft, hop = 16384, 16384 // hd
    y = np.random.default_rng(n_fft + hd + clips).standard_normal((clips, 3 * n_fft + 1)).astype(np.float32)
    kw = dict(n_fft=n_fft, hop_length=hop)
    D, ref = L.stft(y, **kw), O.stft(y, **kw)
    assert D.shape == ref.shape and _stft_close(D, ref)
    for power in (1.0, 2.0, 1.5):
        S, _ = L.core.spectrum._spectrogram(y=y, power=power, **kw)
        Sr, _ = O.spectrogram(y=y, power=power, **kw)
        assert np.abs(S - Sr).max() <= 8e-6 * np.abs(Sr).max(), power


@pytest.mark.parametrize("clips", [1, 2])
@pytest.mark.parametrize("hd", [1, 2, 4, 8])
@pytest.mark.parametrize("n_fft", [1024, 4096, 16384])
def test_second_generation_mel_epilogue_beside_n2048(L, n_fft, hd, clips):
    """Fused mel with 128 bands at n_fft 1024 / 4096 / 16384 and hop = n_fft / {1, 2, 4, 8}: the run-ordered epilogue of the second-generation kernel in
    256-thread (mel) workgroups (csrc/lra_fused.h, instance group 14; n_fft = 2048 has the tests above) -- |X|, |X|^2 and |X|^1.5 on 3 n_fft + 1
    samples, against the oracle at the mel bar."""
    hop = n_fft // hd
    y = np.random.default_rng(n_fft + hd + clips).standard_normal((clips, 3 * n_fft + 1)).astype(np.float32)
    for power in (1.0, 2.0, 1.5):
        kw = dict(y=y, sr=22050, n_fft=n_fft, hop_length=hop, n_mels=128, power=power)
        M, ref = L.feature.melspectrogram(**kw), O.melspectrogram(**kw)
        assert M.shape == ref.shape and not np.isnan(M).any() and _mel_close(M, ref), power


# ---------------------------------------------------------------------------------------------------
# 5. decibel scaling and MFCC
# ---------------------------------------------------------------------------------------------------
# Tolerances: dB values are 10 log10 of float32 powers: one ulp of the logarithm's argument moves the result by 4e-7 dB and
# the device's log10f differs from NumPy's by a few ulp of the RESULT (|dB| <= 150): |d| <= 5e-5 dB.  MFCC sums 40..128
# such values with O(1) weights: |d| <= 2e-4 + 1e-5 |ref|.
DB_TOL = 5e-5


def _mfcc_close(a, ref):
    return np.all(np.abs(a - ref) <= 2e-4 + 1e-5 * np.abs(ref))


def test_db_golden(L):
    g = np.load(os.path.join(GOLDEN_DIR, "db_mfcc.npz"))
    M, A = g["M"], g["A"]
    cases = [
        (L.power_to_db(M), "db_default"),
        (L.power_to_db(M, ref=np.max), "db_refmax"),
        (L.power_to_db(M, top_db=None, amin=1e-6, ref=2.5), "db_notop"),
        (L.power_to_db(M, ref=np.median, top_db=30.0), "db_median_top30"),
        (L.power_to_db(M, ref=np.max, axes=-1, top_db=40.0), "db_axes_last"),
        (L.power_to_db(M, ref=np.max, axes=None), "db_axes_none"),
        (L.amplitude_to_db(A), "adb_default"),
        (L.amplitude_to_db(A, ref=np.max, top_db=60.0), "adb_refmax"),
    ]
    for out, key in cases:
        assert out.shape == g[key].shape and out.dtype == g[key].dtype, key
        assert np.abs(out - g[key]).max() <= DB_TOL, (key, np.abs(out - g[key]).max())
    P = L.db_to_power(g["db_notop"], ref=2.5)
    assert np.all(np.abs(P - g["pow_back"]) <= 2e-6 * np.abs(g["pow_back"]))
    Ab = L.db_to_amplitude(O.amplitude_to_db(A, top_db=None), ref=1.0)
    assert np.all(np.abs(Ab - g["amp_back"]) <= 2e-6 * np.abs(g["amp_back"]) + 1e-12)
    # scalars, 1-d input, float64
    assert abs(float(L.power_to_db(np.float32(0.5))) - float(O.power_to_db(np.float32(0.5)))) <= DB_TOL
    v = np.abs(np.random.default_rng(0).standard_normal(1000)) ** 2
    assert np.abs(L.power_to_db(v, ref=np.max) - O.power_to_db(v, ref=np.max)).max() <= 1e-10
    # real input stays SIGNED in power_to_db (negative values floor at amin; ref / top_db from the signed maximum); amplitude_to_db takes
    # the modulus; array-valued ref broadcasts (core/spectrum.py:1855-1881, 2011-2037)
    import torch
    rng = np.random.default_rng(5)
    X = rng.standard_normal((3, 20, 30)).astype(np.float32)
    neg = -np.abs(X) - 1.0
    refc = np.array([0.5, 2.0, 1e-12])[:, None, None]
    for Xi in (X, neg, X.astype(np.float64)):
        tol = DB_TOL if Xi.dtype == np.float32 else 1e-10
        for kw in (dict(), dict(ref=np.max), dict(ref=np.max, top_db=30.0), dict(top_db=None), dict(ref=np.median), dict(ref=refc), dict(ref=refc.astype(np.float32), top_db=None)):
            got, want = L.power_to_db(Xi, **kw), O.power_to_db(Xi, **kw)
            assert got.shape == want.shape and got.dtype == want.dtype and np.abs(got - want).max() <= tol, (kw, np.abs(got - want).max())
            dev = L.power_to_db(torch.from_numpy(Xi).cuda(), **kw)
            assert dev.is_cuda and np.abs(dev.cpu().numpy() - want).max() <= tol, kw
        for kw in (dict(), dict(ref=np.max), dict(ref=refc, top_db=40.0)):
            got, want = L.amplitude_to_db(Xi, **kw), O.amplitude_to_db(Xi, **kw)
            assert got.dtype == want.dtype and np.abs(got - want).max() <= tol, kw
    dbv = (rng.standard_normal((3, 4, 5)) * 10).astype(np.float32)
    assert np.all(np.abs(L.db_to_power(dbv, ref=refc) - O.db_to_power(dbv, ref=refc)) <= 2e-6 * np.abs(O.db_to_power(dbv, ref=refc)))
    assert np.all(np.abs(L.db_to_amplitude(dbv, ref=refc) - O.db_to_amplitude(dbv, ref=refc)) <= 2e-6 * np.abs(O.db_to_amplitude(dbv, ref=refc)))
    with pytest.raises(L.ParameterError):
        L.power_to_db(X, ref=np.ones((7, 1, 1)))
    with pytest.raises(L.ParameterError):
        L.power_to_db(M, amin=0)
    with pytest.raises(L.ParameterError):
        L.power_to_db(M, top_db=-1)
    with pytest.warns(UserWarning, match="phase"):
        L.power_to_db((M + 1j * M).astype(np.complex64))


def test_mfcc_golden(L):
    g = np.load(os.path.join(GOLDEN_DIR, "db_mfcc.npz"))
    S = g["db_default"]
    for out, key in [
        (L.feature.mfcc(S=S, n_mfcc=13), "mfcc_S"),
        (L.feature.mfcc(S=S, n_mfcc=20, dct_type=3, lifter=22), "mfcc_S_t3_lift"),
        (L.feature.mfcc(S=S, n_mfcc=12, dct_type=1, norm=None), "mfcc_S_t1_none"),
        (L.feature.mfcc(y=g["y"], sr=22050, n_mfcc=20, n_fft=1024, hop_length=256, n_mels=40), "mfcc_y"),
        (L.feature.mfcc(y=g["y2"], sr=22050), "mfcc_y2_default"),
        (L.feature.mfcc(y=g["y2"], sr=22050, n_mfcc=13, lifter=26, htk=True, n_mels=64, fmax=8000.0), "mfcc_y2_htk_lift"),
    ]:
        assert out.shape == g[key].shape and out.dtype == g[key].dtype, key
        assert _mfcc_close(out, g[key]), (key, np.abs(out - g[key]).max())
    with pytest.raises(L.ParameterError):
        L.feature.mfcc(S=S, lifter=-2)


def test_db_mfcc_device_tensors_and_batches(L):
    """Device tensors stay on the device; a batch is scaled per clip (axes="auto"), exactly like clip-by-clip calls."""
    import torch

    yh = O.config_input(3, n=22050 * 2)
    y = torch.from_numpy(yh).cuda()
    M = L.feature.melspectrogram(y=y, sr=22050)
    Mdb = L.power_to_db(M, ref=np.max)
    assert isinstance(Mdb, torch.Tensor) and Mdb.is_cuda and tuple(Mdb.shape) == tuple(M.shape)
    ref = O.power_to_db(O.melspectrogram(y=yh, sr=22050), ref=np.max)
    assert np.abs(Mdb.cpu().numpy() - ref).max() <= 2e-4  # includes the mel kernel's own 1e-6 relative error near the -80 dB floor
    C = L.feature.mfcc(y=y, sr=22050)
    assert isinstance(C, torch.Tensor) and tuple(C.shape) == (3, 20, M.shape[-1])
    Cref = O.mfcc(y=yh, sr=22050)
    assert np.all(np.abs(C.cpu().numpy() - Cref) <= 5e-4 + 1e-5 * np.abs(Cref))
    for i in range(3):
        Ci = L.feature.mfcc(y=yh[i], sr=22050)
        assert np.array_equal(Ci, C[i].cpu().numpy())
    # many coefficients: more than one group of 128 basis rows
    S = torch.randn(2, 200, 50, device="cuda")
    big = L.feature.mfcc(S=S, n_mfcc=150)
    assert _mfcc_close(big.cpu().numpy(), O.mfcc(S=S.cpu().numpy(), n_mfcc=150))


def test_gather_path_under_rccl_world_size_one(L):
    """librosa_amd.distributed on the nccl (= RCCL) backend with device tensors: the collective path bench.py --gpus N uses,
    at world size 1 (the GPU box has one device; two-rank coverage of the same code runs on gloo in tests/test_distributed_cpu.py)."""
    import socket

    import torch
    import torch.distributed as dist

    from librosa_amd.distributed import ShardedGather, chunk_ranges, gather_shards

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group(backend="nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        yh = O.config_input(5, n=22050)
        M = L.feature.melspectrogram(y=torch.from_numpy(yh).cuda(), sr=22050)
        full = gather_shards(M, 5)
        assert full.is_cuda and torch.equal(full, M)
        g = ShardedGather(M, 5)
        for lo, hi in chunk_ranges(5, 3):
            g.push(lo, hi, M[lo:hi])
        assert torch.equal(g.wait(), M)
    finally:
        dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------
# 6. reference edge cases (round-1 review): tests/test_core.py:307-314, 317-371; filters.py:961-977
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", [12, 13, 14, 15, 16])
def test_stft_winsizes_float64(L, power):
    """tests/test_core.py:307-314 (issue #1095): float64, n_fft = 2^12 .. 2^16, hop = n_fft/2, win_length = n_fft.  f64 above
    8192 and anything above 16384 leave the fused kernels for the rocFFT path."""
    N = 2**power
    rng = np.random.default_rng(power)
    x = rng.standard_normal(250000)
    D = L.stft(x, n_fft=N, hop_length=N // 2, win_length=N)
    ref = O.stft(x, n_fft=N, hop_length=N // 2, win_length=N)
    assert D.shape == ref.shape and D.dtype == np.complex128
    assert np.abs(D - ref).max() <= 1e-12 * np.abs(ref).max()
    xz = L.stft(np.zeros(100000), n_fft=N, hop_length=N // 2, win_length=N)  # the reference's own input: all zeros
    assert not xz.any()


def test_window_specifications(L):
    """filters.get_window (filters.py:961-977): name, (name, parameter) tuple, number (Kaiser beta), callable, array, list."""
    rng = np.random.default_rng(5)
    y = rng.standard_normal(6000).astype(np.float32)
    import scipy.signal

    vec = scipy.signal.get_window("hamming", 512, fftbins=True)
    for window in ("hamming", ("kaiser", 4.0), ("tukey", 0.25), 4.0, (lambda n: np.bartlett(n)), vec, list(vec)):
        D = L.stft(y, n_fft=512, hop_length=128, window=window)
        ref = O.stft(y, n_fft=512, hop_length=128, window=window)
        assert _stft_close(D, ref), window
        yy = L.istft(D, hop_length=128, window=window, length=len(y))
        assert np.abs(yy - O.istft(ref, hop_length=128, window=window, length=len(y))).max() <= 2e-5, window
    with pytest.raises(L.ParameterError):
        L.stft(y, n_fft=512, window=vec[:100])
    with pytest.raises(L.ParameterError):
        L.stft(y, n_fft=512, window={"not": "a window"})


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("n_fft,hop_length", [(1023, 128), (1023, 129), (1023, 256), (2048, 512), (2048, 2048)])
@pytest.mark.parametrize("N", [1024, 2048, 8192])
def test_stft_preallocate(L, center, n_fft, hop_length, N):
    """tests/test_core.py:317-371: stereo, out= exact / oversize (the same object or out[..., :n_frames] comes back) / undersize."""
    rng = np.random.default_rng(N + n_fft + hop_length)
    y = rng.standard_normal(size=(2, max(N, n_fft)))
    D1 = L.stft(y, center=center, n_fft=n_fft, hop_length=hop_length)
    assert np.abs(D1 - O.stft(y, center=center, n_fft=n_fft, hop_length=hop_length)).max() <= 1e-12 * max(1.0, np.abs(D1).max())
    out = np.empty_like(D1)
    D2 = L.stft(y, center=center, n_fft=n_fft, hop_length=hop_length, out=out)
    assert D2 is out and np.array_equal(D1, D2)
    if N == 2048:
        shape = list(D1.shape)
        shape[-1] *= 2
        big = np.empty_like(D1, shape=shape)
        D3 = L.stft(y, center=center, n_fft=n_fft, hop_length=hop_length, out=big)
        assert np.array_equal(D1, D3) and np.array_equal(D1, big[..., : D3.shape[-1]]) and np.shares_memory(D3, big)
        shape[-1] = max(1, D1.shape[-1] // 2)
        if shape[-1] < D1.shape[-1]:
            with pytest.raises(L.ParameterError):
                L.stft(y, center=center, n_fft=n_fft, hop_length=hop_length, out=np.empty_like(D1, shape=shape))


def test_istft_bins_follow_n_fft_like_irfft(L):
    """An explicit n_fft that disagrees with the matrix: irfft(n=n_fft) crops / zero-pads the bin axis (core/spectrum.py:566, 598)."""
    rng = np.random.default_rng(9)
    y = rng.standard_normal(5000).astype(np.float32)
    D = O.stft(y, n_fft=1024, hop_length=256)
    for n_fft in (512, 2048):
        got = L.istft(D, n_fft=n_fft, hop_length=256)
        ref = O.istft(D, n_fft=n_fft, hop_length=256)
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())


# ---- Griffin-Lim (librosa/core/spectrum.py:2669-2917) ------------------------------------------------
def _spectral_convergence(y, S, skw):
    """|| |stft(y)| - S || / || S ||  (the quantity Griffin-Lim descends on), evaluated with the oracle."""
    R = np.abs(O.stft(y, **skw))
    return float(np.linalg.norm(R - S) / np.linalg.norm(S))


def test_griffinlim_update_kernel(L):
    """The phase update follows NumPy's complex64 loops operation by operation (lra_post.h)."""
    import torch

    rng = np.random.default_rng(5)
    ctx = L.get_context(0)
    for real, cplx in ((np.float32, np.complex64), (np.float64, np.complex128)):
        n = 100003
        rebuilt = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(cplx)
        tprev = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(cplx)
        rebuilt[:7] = 0  # |angles| = 0: the eps in the denominator decides
        tprev[:3] = 0
        S = np.abs(rng.standard_normal(n)).astype(real)
        eps = float(np.finfo(real).tiny)
        for mom, prev in ((0.99, tprev), (0.3, tprev), (0.99, None)):
            ref = O.griffinlim_update(rebuilt, prev, S, mom, np.finfo(real).tiny)
            r, s = torch.from_numpy(rebuilt).cuda(), torch.from_numpy(S).cuda()
            t = torch.from_numpy(prev).cuda() if prev is not None else None
            out = torch.empty_like(r)
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            ctx.griffinlim_update(r.data_ptr(), t.data_ptr() if t is not None else None, s.data_ptr(), out.data_ptr(), n, real, mom / (1 + mom), eps)
            got = out.cpu().numpy()
            # NumPy's |complex64| is a float32 hypot whose last bit depends on the host's SIMD dispatch; the kernel's is the
            # correctly rounded one, everything else follows NumPy's operation order (the last-bit difference of |.| passes through
            # a reciprocal and two products)
            assert np.all(np.abs(got.real - ref.real) <= 4 * np.finfo(real).eps * np.abs(ref.real)), (mom, prev is None)
            assert np.all(np.abs(got.imag - ref.imag) <= 4 * np.finfo(real).eps * np.abs(ref.imag)), (mom, prev is None)


@pytest.mark.parametrize("name", list(golden_cases.GRIFFINLIM_CASES))
def test_griffinlim_golden(L, name):
    """Against the reference's own output for the same seed.  The iteration is a fixed-point map, not a contraction: a
    float32 FFT's 1e-7 differences grow by a small factor per round where |angles| is tiny, so the sample-wise bar is
    loose and scaled by the iteration count; the quantity the algorithm minimises must match the reference's closely."""
    g = np.load(os.path.join(GOLDEN_DIR, "griffinlim.npz"))
    case = golden_cases.GRIFFINLIM_CASES[name]
    S, ref = g[f"{name}__S"], g[f"{name}__y"]
    y = L.griffinlim(S, **case["gl"])
    assert y.shape == ref.shape and y.dtype == ref.dtype
    n_iter = case["gl"]["n_iter"]
    err = np.abs(y - ref).max() / np.abs(ref).max()
    if y.dtype == np.float64:
        assert err <= 1e-9, err
    else:
        assert err <= (2e-4 if n_iter <= 8 else 5e-2), err
    skw = dict(case["stft"])
    c_ref, c_got = _spectral_convergence(ref, S, skw), _spectral_convergence(y, S, skw)
    assert abs(c_got - c_ref) <= 0.02 * c_ref + 1e-6, (c_got, c_ref)


@pytest.mark.parametrize("n_fft", [2048, 2049])
@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("use_length", [False, True])
@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("init", [None, "random"])
def test_griffinlim_reference_matrix(L, n_fft, center, use_length, pad_mode, init):
    """tests/test_core.py:2583-2640 (hop / win_length / window folded into two combinations per case)."""
    y = golden_cases.make_signal("chirp", 22050, 41, None, "float32")
    for hop_length, win_length, window in ((None, None, "hann"), (1024, 1024, "boxcar")):
        S = np.abs(O.stft(y, hop_length=hop_length, win_length=win_length, n_fft=n_fft, window=window, center=center, pad_mode=pad_mode))
        kw = dict(hop_length=hop_length, win_length=win_length, n_fft=n_fft, window=window, center=center, length=len(y) if use_length else None, pad_mode=pad_mode, n_iter=1, init=init)
        y_rec = L.griffinlim(S, rng=0, **kw)
        if use_length:
            assert len(y_rec) == len(y)
        assert np.isrealobj(y_rec) and np.all(np.isfinite(y_rec))
        ref = O.griffinlim(S, rng=0, **kw)
        assert y_rec.shape == ref.shape
        well = _wss_for(dict(n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window, center=center), S.shape[-1], ref.shape[-1], kw["length"], np.float32)
        well = well > 1e-2 * well.max()
        # init=None starts from zero phases: the first rebuilt spectrum is full of near-cancellations, whose normalisation
        # (angles / |angles|) amplifies float32 rounding
        assert np.abs(y_rec - ref)[well].max() <= (1e-4 if init == "random" else 2e-3) * np.abs(ref).max()


def test_pcg64_device_stream_is_numpys(L):
    """csrc/lra_rng.h on the device: draws offset .. offset + count of np.random.default_rng(seed).random(), bit for bit (integer arithmetic + one exact
    conversion), for several seeds / sizes / jump-ahead offsets; then griffinlim with device-drawn phases against the host-drawn path (same values, and
    the caller's generator left in the same state)."""
    import torch
    from librosa_amd.core import spectrum as SP

    ctx = L.get_context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for seed in (0, 7, 440, 2**64 + 3):
        for offset, count in ((0, 1), (0, 1000), (5, 129), (123457, 4096), (2**33 + 1, 777), (0, 3_000_001)):
            g = np.random.default_rng(seed)
            st = g.bit_generator.state["state"]
            out = torch.empty(count, dtype=torch.float64, device="cuda")
            ctx.pcg64_random_exec(st["state"], st["inc"], offset, out.data_ptr(), count)
            g.bit_generator.advance(offset)
            assert np.array_equal(out.cpu().numpy(), g.random(count)), (seed, offset, count)
    y = golden_cases.make_signal("mix", 22050, 3, (2,), "float32")
    S = np.abs(L.stft(y, n_fft=1024, hop_length=256))
    for dtype in (np.float32, np.float64):
        g1, g2 = np.random.default_rng(99), np.random.default_rng(99)
        a = L.griffinlim(S.astype(dtype), n_iter=3, hop_length=256, rng=g1)
        old = SP.DEVICE_RNG
        SP.DEVICE_RNG = False
        try:
            b = L.griffinlim(S.astype(dtype), n_iter=3, hop_length=256, rng=g2)
        finally:
            SP.DEVICE_RNG = old
        assert np.array_equal(a, b)
        assert g1.bit_generator.state == g2.bit_generator.state and g1.random() == g2.random()
    # a generator with a cached 32-bit half (an odd number of 32-bit draws behind it) keeps that half, as with the reference's rng.random() ...
    g1, g2 = np.random.default_rng(5), np.random.default_rng(5)
    for g in (g1, g2):
        g.integers(0, 2**31, dtype=np.uint32)
        assert g.bit_generator.state["has_uint32"] == 1
    L.griffinlim(S, n_iter=1, hop_length=256, rng=g1)
    g2.random(size=S.shape)
    assert g1.bit_generator.state == g2.bit_generator.state
    assert g1.integers(0, 2**31, dtype=np.uint32) == g2.integers(0, 2**31, dtype=np.uint32) and g1.random() == g2.random()
    # ... and a call that fails before the draws are taken leaves the generator where it was
    g3 = np.random.default_rng(11)
    before = g3.bit_generator.state
    with pytest.raises(L.ParameterError):
        L.griffinlim(S, n_iter=1, hop_length=256, n_fft=1024, length=17, rng=g3)
    assert g3.bit_generator.state == before
    # other bit generators and RandomState keep the host path
    r1 = L.griffinlim(S, n_iter=2, hop_length=256, rng=np.random.Generator(np.random.Philox(5)))
    r2 = L.griffinlim(S, n_iter=2, hop_length=256, rng=np.random.Generator(np.random.Philox(5)))
    assert np.array_equal(r1, r2) and np.isfinite(r1).all()


def test_griffinlim_arguments(L):
    """tests/test_core.py:2643-2711: dtype, momentum, rng state, deprecated random_state, error paths."""
    import torch

    y = golden_cases.make_signal("chirp", 22050, 42, None, "float32")
    S = np.abs(O.stft(y))
    for dt in (np.float32, np.float64):
        assert L.griffinlim(S, dtype=dt, n_iter=1).dtype == dt
    for momentum in (0, 0.99):
        L.griffinlim(S, momentum=momentum, n_iter=1)
    a, b = L.griffinlim(S, rng=0, n_iter=1), L.griffinlim(S, rng=0, n_iter=1)
    assert np.array_equal(a, b)
    L.griffinlim(S, rng=np.random.RandomState(), n_iter=1)
    with pytest.warns(FutureWarning, match="renamed to 'rng'"):
        y1 = L.griffinlim(S, n_iter=2, random_state=5)
    assert np.array_equal(y1, L.griffinlim(S, n_iter=2, rng=5))
    x = np.zeros((33, 3))
    with pytest.raises(L.ParameterError):
        L.griffinlim(x, init="garbage")
    with pytest.raises(TypeError):
        L.griffinlim(x, rng="garbage")
    with pytest.raises(L.ParameterError):
        L.griffinlim(x, rng=0, random_state=0)
    with pytest.raises(L.ParameterError):
        L.griffinlim(x, momentum=-1)
    with pytest.warns(UserWarning):
        z = L.griffinlim(x, momentum=2)
    assert z.shape == (32,) and z.dtype == np.float64 and np.all(z == 0)
    # device tensors: same numbers, nothing leaves the device
    St = torch.from_numpy(S).cuda()
    yt = L.griffinlim(St, rng=3, n_iter=4)
    assert isinstance(yt, torch.Tensor) and yt.is_cuda
    assert np.array_equal(yt.cpu().numpy(), L.griffinlim(S, rng=3, n_iter=4))
    # a batch is processed clip by clip with one stream of random phases, exactly like the reference
    Sb = np.stack([S, 0.5 * S])
    yb = L.griffinlim(Sb, rng=1, n_iter=3)
    assert np.abs(yb - O.griffinlim(Sb, rng=1, n_iter=3)).max() <= 2e-4 * np.abs(yb).max()


# ---- NumPy drop-in through the native host pipeline; streaming ----------------------------------------
def test_host_pipeline_chunking_and_finite_scan(L):
    """lra_stft_exec_host: any staging granularity gives the same numbers as one device-resident call; the staging threads'
    finite scan finds a single bad sample anywhere (util.valid_audio, util/utils.py:305)."""
    import torch

    ctx = L.get_context(0)
    y = O.config_input(11, n=40000)
    y64 = y.astype(np.float64)
    try:
        for mb in (1, 2, 128):
            ctx.set_option("pipe_chunk_mb", mb)
            D = L.stft(y, n_fft=1024, hop_length=256)
            assert np.array_equal(D, L.stft(torch.from_numpy(y).cuda(), n_fft=1024, hop_length=256).cpu().numpy())
            M = L.feature.melspectrogram(y=y, sr=22050, n_fft=1024, hop_length=256, n_mels=40)
            assert np.array_equal(M, L.feature.melspectrogram(y=torch.from_numpy(y).cuda(), sr=22050, n_fft=1024, hop_length=256, n_mels=40).cpu().numpy())
            S, _ = L._spectrogram(y=y, n_fft=1024, hop_length=256, power=1)
            assert _stft_close(S.astype(np.complex64), np.abs(O.stft(y, n_fft=1024, hop_length=256)).astype(np.complex64))
            D64 = L.stft(y64, n_fft=1000, hop_length=250)  # rocFFT path, float64
            assert _stft_close(D64, O.stft(y64, n_fft=1000, hop_length=250))
            # inverse through lra_istft_exec_host (frame-major spectrum, as stft returns it) == the device-tensor path
            yi = L.istft(D, hop_length=256, length=y.shape[-1])
            assert np.array_equal(yi, L.istft(torch.from_numpy(np.ascontiguousarray(D)).cuda(), hop_length=256, length=y.shape[-1]).cpu().numpy())
            pre = np.zeros_like(yi)
            assert L.istft(D, hop_length=256, length=y.shape[-1], out=pre) is pre and np.array_equal(pre, yi)
            assert np.array_equal(L.istft(np.ascontiguousarray(D), hop_length=256, length=y.shape[-1]), yi)  # C-ordered spectrum: device transposition
            assert np.abs(L.istft(D64, hop_length=250, n_fft=1000, length=y.shape[-1]) - y64).max() <= 1e-9
        ctx.set_option("pipe_chunk_mb", 1)
        for b, i in ((0, 0), (10, 39999), (5, 20001)):
            for v in (np.nan, np.inf, -np.inf):
                bad = y.copy()
                bad[b, i] = v
                with pytest.raises(L.ParameterError, match="not finite"):
                    L.stft(bad, n_fft=1024, hop_length=256)
                with pytest.raises(L.ParameterError, match="not finite"):
                    L.feature.melspectrogram(y=bad.astype(np.float64), sr=22050, n_fft=512, hop_length=2000)  # hop > n_fft: no frame sees every sample
        big = y.copy()
        big[3, 7] = 3e38  # finite: overflows the DC bin, but valid_audio looks at the samples
        assert L.stft(big, n_fft=1024, hop_length=256).shape == D.shape
    finally:
        ctx.set_option("pipe_chunk_mb", 128)
    # non-contiguous / strided input
    ys = np.asfortranarray(y)
    assert np.array_equal(L.stft(ys, n_fft=1024, hop_length=256), D)


def test_streaming_stft_out_reuse(L):
    """docs/examples/plot_pcen_stream.py:72-74: D = stft(block, center=False, out=D) over librosa.stream blocks; the output
    array and every staging / device buffer are reused from the second block on, and the tiled frames are the STFT of the
    whole signal."""
    n_fft, hop, block_length = 2048, 512, 16
    y = O.config_input(1, n=22050 * 4)[0]
    whole = O.stft(y, n_fft=n_fft, hop_length=hop, center=False)
    D, cols, ident = None, [], []
    for blk in L.stream(y, block_length=block_length, frame_length=n_fft, hop_length=hop, fill_value=0.0):
        D2 = L.stft(blk, n_fft=n_fft, hop_length=hop, center=False, out=D)
        ident.append(D is None or D2 is D)
        D = D2
        cols.append(D.copy())
    assert all(ident) and D.shape == (1025, block_length)
    tiled = np.concatenate(cols, axis=-1)[:, : whole.shape[1]]
    assert _stft_close(tiled, whole)
    # the reference's preallocation matrix: wider out, C-ordered out, wrong shapes (tests/test_core.py:317-371)
    blk = y[: (block_length - 1) * hop + n_fft]
    ref = O.stft(blk, n_fft=n_fft, hop_length=hop, center=False)
    wide_f = np.zeros((1025, block_length + 5), dtype=np.complex64, order="F")
    r = L.stft(blk, n_fft=n_fft, hop_length=hop, center=False, out=wide_f)
    assert r.shape == ref.shape and np.shares_memory(r, wide_f) and _stft_close(r, ref) and np.all(wide_f[:, block_length:] == 0)
    wide_c = np.zeros((1025, block_length + 5), dtype=np.complex64)
    r = L.stft(blk, n_fft=n_fft, hop_length=hop, center=False, out=wide_c)
    assert np.shares_memory(r, wide_c) and _stft_close(r, ref)
    out128 = np.zeros((1025, block_length), dtype=np.complex128)
    r = L.stft(blk, n_fft=n_fft, hop_length=hop, center=False, out=out128)
    assert r is out128 and _stft_close(r.astype(np.complex64), ref)
    stereo = np.stack([blk, -blk])
    outs = np.zeros((2, 1025, block_length + 1), dtype=np.complex64)
    r = L.stft(stereo, n_fft=n_fft, hop_length=hop, center=False, out=outs)
    assert np.shares_memory(r, outs) and _stft_close(r[0], ref) and _stft_close(r[1], -ref)
    with pytest.raises(L.ParameterError):
        L.stft(blk, n_fft=n_fft, hop_length=hop, center=False, out=np.zeros((1025, block_length - 1), dtype=np.complex64))
    with pytest.raises(L.ParameterError):
        L.stft(blk, n_fft=n_fft, hop_length=hop, center=False, out=np.zeros((1025, block_length), dtype=np.float32))


@pytest.mark.parametrize("n_fft,hop,center,pad_mode,dtype", [(512, 512, True, "constant", np.float32), (512, 512, False, "constant", np.float32), (256, 300, True, "reflect", np.float32),
                                                            (2048, 2048, True, "edge", np.float32), (8192, 8192, True, "symmetric", np.float32), (128, 1000, True, "constant", np.float32),
                                                            (512, 512, True, "reflect", np.float64), (4096, 5000, False, "constant", np.float64)])
def test_direct_framing(L, n_fft, hop, center, pad_mode, dtype):
    """hop >= n_fft (BASELINE configs[4]'s n_fft = 512 leg): frames do not overlap and the kernels frame without a ring
    (stft_kernel<..., RA = 2>); with the option off the ring kernels must give the same numbers."""
    ctx = L.get_context(0)
    rng = np.random.default_rng(n_fft + hop)
    y = rng.standard_normal((3, 70001)).astype(dtype)  # odd length: clips 1.. start on odd sample addresses
    ref = O.stft(y, n_fft=n_fft, hop_length=hop, center=center, pad_mode=pad_mode)
    try:
        for v2 in (1, 0):
            ctx.set_option("v2", v2)
            D = L.stft(y, n_fft=n_fft, hop_length=hop, center=center, pad_mode=pad_mode)
            assert D.shape == ref.shape and _stft_close(D, ref)
            S, _ = L._spectrogram(y=y, n_fft=n_fft, hop_length=hop, power=2, center=center, pad_mode=pad_mode)
            assert np.all(np.abs(S - np.abs(ref) ** 2) <= (1e-11 if dtype == np.float64 else 4e-6) * (np.abs(ref) ** 2).max())
        ctx.set_option("direct", 0)
        assert _stft_close(L.stft(y, n_fft=n_fft, hop_length=hop, center=center, pad_mode=pad_mode), ref)
    finally:
        ctx.set_option("v2", 1)
        ctx.set_option("direct", 1)


def test_long_clip_shards_by_frames_in_process(L, monkeypatch):
    """a call with fewer clips than devices shards ONE long clip by FRAMES (distributed.shard_frames: each device the uncentred
    transform of its sample range + halo, the centre padding on the first / last shard).  On the 1-GPU box both ranges run on device 0; stft (incl.
    out= with spare columns), _spectrogram and melspectrogram must equal the unsharded call bit for bit, for every pad mode, and a non-finite sample in the
    last shard must still raise.  Reference: core/spectrum.py:273-328, 380-390."""
    from librosa_amd.core import spectrum

    y = golden_cases.make_signal("noise", 22050 * 8, 21, (1,))
    n_dev = L.device_count()
    two = ",".join(str(i % n_dev) for i in range(2)) if n_dev < 2 else "all"
    for n_fft, hop, center, pad_mode in ((2048, 512, True, "constant"), (2048, 512, True, "reflect"), (1024, 256, False, "constant"), (512, 160, True, "symmetric"), (400, 160, True, "edge"), (1200, 300, True, "reflect")):
        # (the mixed-radix kernels unroll their stages over work items: a frame's bits must not depend on the copy of the body it lands in -- 400 / 160 and 1200 / 300)
        kw = dict(n_fft=n_fft, hop_length=hop, center=center, pad_mode=pad_mode)
        monkeypatch.setenv("LRA_DEVICES", "0")
        D1 = L.stft(y, **kw)
        S1, _ = spectrum._spectrogram(y=y, power=2, **kw)
        M1 = L.feature.melspectrogram(y=y, sr=22050, n_mels=64, **kw)
        monkeypatch.setattr(spectrum, "_MULTI_DEVICE_MIN_BYTES", 0)
        monkeypatch.setattr(spectrum, "_FRAME_SHARD_MIN_FRAMES", 8)
        monkeypatch.setenv("LRA_DEVICES", two)
        served = []
        orig = spectrum._frame_sharded_host_exec
        monkeypatch.setattr(spectrum, "_frame_sharded_host_exec", lambda sess, shards, run: (served.extend(sh for _, sh in shards if isinstance(sh, dict)), orig(sess, shards, run))[1])
        D2 = L.stft(y, **kw)
        assert len(served) >= 2 and served[0]["frame_lo"] == 0 and served[-1]["frame_hi"] == D1.shape[-1]
        assert np.array_equal(D1, D2)
        assert np.array_equal(S1, spectrum._spectrogram(y=y, power=2, **kw)[0])
        assert np.array_equal(M1, L.feature.melspectrogram(y=y, sr=22050, n_mels=64, **kw))
        out = np.swapaxes(np.zeros((1, D1.shape[-1] + 5, D1.shape[-2]), dtype=np.complex64), -1, -2)
        got = L.stft(y, out=out, **kw)
        assert np.array_equal(got, D1) and np.shares_memory(got, out)
        # the inverse by OUTPUT-sample ranges (each device: the frames that reach into its samples, its piece of the window sum-square envelope)
        ikw = dict(hop_length=hop, n_fft=n_fft, center=center)
        for length in (None, y.shape[-1], y.shape[-1] - 777):
            monkeypatch.setenv("LRA_DEVICES", "0")
            y1 = L.istft(D1, length=length, **ikw)
            monkeypatch.setenv("LRA_DEVICES", "0,0,0")
            assert spectrum._istft_sample_shards(y1.shape[-1], D1.shape[-1], 1, 1 << 40, n_fft, hop, center) is not None
            assert np.array_equal(y1, L.istft(D1, length=length, **ikw)), (n_fft, hop, center, length)
        monkeypatch.setenv("LRA_DEVICES", two)
        y2 = np.stack([y[0], -y[0][::-1]])  # two clips on three "devices": still fewer than two per device
        monkeypatch.setenv("LRA_DEVICES", "0,0,0")
        D3 = L.stft(y2, **kw)
        monkeypatch.setenv("LRA_DEVICES", "0")
        assert np.array_equal(D3, L.stft(y2, **kw))
        monkeypatch.setattr(spectrum, "_frame_sharded_host_exec", orig)
    monkeypatch.setenv("LRA_DEVICES", two)
    bad = y.copy()
    bad[0, -5] = np.inf
    with pytest.raises(L.ParameterError):
        L.stft(bad, n_fft=2048, hop_length=512)


@pytest.mark.parametrize("hop,center,length", [(512, True, "n"), (512, True, None), (1024, False, None), (256, True, 50000), (128, True, "n")])
def test_istft_16_byte_loads(L, hop, center, length):
    """ctx option istft16 (variant 7: the inverse as radices 4, 16, 16 -- four first-pass butterflies per thread, the spectrum row read as 16-byte pieces; csrc/lra_kernels.h
    istft_unsplit_pass0_mir4): against the oracle like the default form, NaN-prefilled output, and against the default form.  librosa/core/spectrum.py:506-626."""
    import torch
    ctx = L.get_context(0)
    y = np.random.default_rng(hop).standard_normal((3, 70001)).astype(np.float32)
    D = O.stft(y, n_fft=2048, hop_length=hop, center=center)
    ln = y.shape[-1] if length == "n" else length
    ref = O.istft(D, hop_length=hop, n_fft=2048, center=center, length=ln)
    wss = _wss_for(dict(n_fft=2048, hop_length=hop, center=center), D.shape[-1], ref.shape[-1], ln, ref.dtype)
    try:
        ctx.set_option("istft16", 1)
        yh = L.istft(D, hop_length=hop, n_fft=2048, center=center, length=ln)
        assert yh.shape == ref.shape and _istft_close(yh, ref, wss)
        yt = L.istft(torch.from_numpy(D).to("cuda:0"), hop_length=hop, n_fft=2048, center=center, length=ln).cpu().numpy()
        assert np.array_equal(yt, yh)
        ctx.set_option("istft16", 0)
        y0 = L.istft(D, hop_length=hop, n_fft=2048, center=center, length=ln)
        assert _istft_close(yh, y0, wss)
    finally:
        ctx.set_option("istft16", 0)


def test_placed_buffers_stay_coherent_under_churn(L):
    """Regression (round 6): with losing candidates' address ranges freed (hipMemAddressFree) or re-used, OTHER live placed buffers were read with stale contents on ROCm 7.0 --
    the fourth of four live tensors gave back its placement probe's values after fill_, two live stft results differed from the torch.empty result in 10^8 values
    (scripts/vmm_coherence.hip reproduces it without this library).  lra_malloc_placed now never re-uses or frees a range while the context lives.  Several placed tensors
    alive at once, released and re-allocated in between, every one must keep exactly what was written to it -- read by kernels AND by a device-to-host copy."""
    import gc

    import torch
    from librosa_amd import _arrays
    ctx = L.get_context(0)
    old = ctx.placement_retry
    try:
        ctx.set_option("placement_retry", 4)
        shape = (24, 2584, 1025)   # 508 MB each
        live = []
        for rnd in range(4):
            for _ in range(3):
                t = _arrays._placed_tensor(ctx, shape, np.dtype(np.complex64), "cuda:0")
                t.fill_(complex(len(live) + 1 + 10 * rnd, 0))
                live.append((t, len(live) + 1 + 10 * rnd))
            torch.cuda.synchronize()
            for t, v in live:
                assert float(t.real.min()) == v and float(t.real.max()) == v and float(t.imag.abs().max()) == 0.0, (rnd, v)
                assert complex(t[0, 0, 0].cpu()) == complex(v, 0) and complex(t[-1, -1, -1].cpu()) == complex(v, 0)
            del live[::2]
            gc.collect()
            ctx.placed_release_all()     # their physical memory goes back: the survivors must not notice
            live = [(t, v) for t, v in live]
            for t, v in live:
                t.fill_(complex(v, 0))
        # the public path: results on placed buffers, several alive at once, against the torch.empty path
        y = torch.from_numpy(O.config_input(48, n=22050 * 30)).to("cuda:0")
        ctx.set_option("placement_retry", 0)
        ref = L.stft(y, n_fft=2048, hop_length=512)
        ctx.set_option("placement_retry", 4)
        outs = [L.stft(y, n_fft=2048, hop_length=512) for _ in range(4)]
        assert all(torch.equal(o, ref) for o in outs)
    finally:
        ctx.set_option("placement_retry", old)
        live = outs = None
        gc.collect()
        ctx.placed_release_all()


def test_placed_result_buffers(L):
    """ctx option placement_retry (include/librosa_amd.h, lra_malloc_placed): a large stft(<device tensor>) result comes from the best of a few candidate
    allocations, wrapped as an ordinary tensor; the values are those of an ordinary result, the buffer is recycled when the tensor dies (same pointer for the
    next call of that shape), and the raw API refuses what it cannot judge."""
    import ctypes
    import gc

    import torch
    ctx = L.get_context(0)
    y = torch.from_numpy(O.config_input(48, n=22050 * 30)).to("cuda:0")   # 48 x 1292 x 1025 complex64 = 508 MB
    old = ctx.placement_retry
    ctx.set_option("placement_retry", 0)
    ref = L.stft(y, n_fft=2048, hop_length=512)   # torch's allocator
    try:
        ctx.set_option("placement_retry", 3)
        D = L.stft(y, n_fft=2048, hop_length=512)
        assert ctx._placed_log and ctx._placed_log[-1][0] == 48 * 1292 * 1025 * 8 and 1 <= ctx._placed_log[-1][3] <= 3 and ctx._placed_log[-1][2] > 0
        assert torch.equal(D, ref) and D.shape == ref.shape and D.dtype == ref.dtype
        n_alloc = len(ctx._placed_log)
        ptr = D.data_ptr()
        S = D.abs().sum()  # ordinary tensor arithmetic on the placed buffer
        assert torch.isfinite(S)
        del D
        gc.collect()
        D2 = L.stft(y, n_fft=2048, hop_length=512)
        assert D2.data_ptr() == ptr and len(ctx._placed_log) == n_alloc and torch.equal(D2, ref)   # recycled, not re-allocated
        view = D2[3]            # a view keeps the buffer alive
        del D2
        gc.collect()
        D3 = L.stft(y, n_fft=2048, hop_length=512)
        assert D3.data_ptr() != ptr and torch.equal(view, ref[3])
        del D3, view
        gc.collect()
        small = L.stft(y[:2], n_fft=2048, hop_length=512)    # below 256 MB: torch's allocator as before
        assert len(ctx._placed_log) == n_alloc + 1 and torch.equal(small, ref[:2])
        # the inverse transform's output is placed too (its rate follows where its OUTPUT lands): a result without a row structure, judged as 8 KiB rows
        y2 = torch.cat([y, y, y[:8]])                                  # 104 clips: 275 MB of samples
        D104 = L.stft(y2, n_fft=2048, hop_length=512)
        n_alloc = len(ctx._placed_log)
        yh = L.istft(D104, hop_length=512, length=y2.shape[-1])
        assert len(ctx._placed_log) == n_alloc + 1 and ctx._placed_log[-1][1] == 8192 and yh.shape == y2.shape and yh.is_contiguous()
        err = ((y2 - yh).double() ** 2).sum(-1)
        assert float((10 * torch.log10((y2.double() ** 2).sum(-1) / err)).min()) >= 60.0
        ctx.set_option("placement_retry", 0)
        assert torch.equal(yh, L.istft(D104, hop_length=512, length=y2.shape[-1]))
        ctx.set_option("placement_retry", 3)
        del D104, yh, y2
        gc.collect()
        p = ctypes.c_void_p()
        assert ctx.lib.lra_malloc_placed(ctx.handle, 1 << 20, 8200, 0, 2, ctypes.byref(p), None, None) != 0   # too few rows to judge
        assert ctx.lib.lra_free_placed(ctx.handle, ctypes.c_void_p(12345)) != 0
    finally:
        ctx.set_option("placement_retry", old)
        gc.collect()
        ctx.placed_release_all()


# ---- round 6: the two new forms of the n_fft = 2048 forward kernels, switched on by context options ---------------------------------------------
@pytest.mark.parametrize("hop,power,n,batch", [(512, 2.0, 22050, 2), (512, 2.0, 9000, 3), (512, 2.0, 661500, 5), (256, 2.0, 100000, 4), (256, 1.0, 100000, 4), (512, 2.0, 2048, 1), (512, 2.0, 70001, 7)])
def test_producer_consumer_mel_kernel(L, hop, power, n, batch):
    """ctx option mel_pc (csrc/lra_kernels_pc.h: 192-thread workgroups [P, P, C], the power row handed from the FFT waves to the mel wave through LDS flags):
    against the oracle at the pure-relative bar on noise-floored input, against the one-wave kernel at rounding level, every output element stored
    (the result buffer starts as NaN).  librosa/feature/spectral.py:2158-2160."""
    import torch
    ctx = L.get_context(0)
    y = O.config_input(batch, n=n)
    ref = O.melspectrogram(y=y, sr=22050, n_fft=2048, hop_length=hop, n_mels=128, power=power)
    yt = torch.from_numpy(y).to("cuda:0")
    try:
        outs = []
        for pc in (0, 1):
            ctx.set_option("mel_pc", pc)
            M = L.feature.melspectrogram(y=yt, sr=22050, n_fft=2048, hop_length=hop, n_mels=128, power=power).cpu().numpy()
            assert M.shape == ref.shape and not np.isnan(M).any()
            assert np.all(np.abs(M - ref) <= 1e-4 * np.abs(ref)), (pc, float(np.max(np.abs(M - ref) / np.abs(ref))))
            outs.append(M)
        assert np.all(np.abs(outs[1] - outs[0]) <= 2e-5 * np.abs(outs[0]))  # (two float32 kernels: same operations, different fused-multiply-add contraction)
        # NumPy drop-in through the host pipeline with the option on
        ctx.set_option("mel_pc", 1)
        Mh = L.feature.melspectrogram(y=y, sr=22050, n_fft=2048, hop_length=hop, n_mels=128, power=power)
        assert np.array_equal(Mh, outs[1])
    finally:
        ctx.set_option("mel_pc", 1)  # (the library's default)


def test_producer_consumer_mel_kernel_full_size(L, full_batch):
    """BASELINE configs[1] through the producer / consumer kernel: 256 clips x 30 s, four clips at the pure-relative bar, per-clip independence (clip i of the
    batch == clip i alone), and banks it does not serve (40 bands: segments wider than its register lists) still answered by the one-wave kernel."""
    import torch
    ctx = L.get_context(0)
    yt = full_batch
    try:
        ctx.set_option("mel_pc", 1)
        M = L.feature.melspectrogram(y=yt, sr=22050, n_fft=2048, hop_length=512, n_mels=128)
        assert not bool(torch.isnan(M).any())
        for i in (0, 71, 128, 255):
            ref = O.melspectrogram(y=yt[i].cpu().numpy(), sr=22050, n_fft=2048, hop_length=512, n_mels=128)
            got = M[i].cpu().numpy()
            assert np.all(np.abs(got - ref) <= 1e-4 * np.abs(ref)), i
            assert np.array_equal(L.feature.melspectrogram(y=yt[i], sr=22050, n_fft=2048, hop_length=512, n_mels=128).cpu().numpy(), got)
        M40 = L.feature.melspectrogram(y=yt[:3], sr=22050, n_fft=2048, hop_length=512, n_mels=40).cpu().numpy()
        ctx.set_option("mel_pc", 0)
        assert np.array_equal(M40, L.feature.melspectrogram(y=yt[:3], sr=22050, n_fft=2048, hop_length=512, n_mels=40).cpu().numpy())
    finally:
        ctx.set_option("mel_pc", 1)  # (the library's default)


@pytest.mark.parametrize("hop,center,pad_mode,n", [(512, True, "constant", 22050), (512, True, "reflect", 9000), (256, True, "edge", 100000), (1024, False, "constant", 100000), (2048, True, "symmetric", 50000),
                                                   (512, True, "constant", 2048), (512, False, "constant", 70001)])
def test_radix_16_16_4_forward(L, hop, center, pad_mode, n):
    """ctx option v3 (variant 6: radices 16, 16, 4 -- neighbouring bins side by side in one thread, the row leaving as 16-byte pieces): stft and
    _spectrogram against the oracle, packed rows and rows padded to 128-byte lines, NaN-poisoned padding untouched.  librosa/core/spectrum.py:356, 380-390."""
    import torch
    ctx = L.get_context(0)
    y = np.random.default_rng(hop + n).standard_normal((3, n)).astype(np.float32)
    ref = O.stft(y, n_fft=2048, hop_length=hop, center=center, pad_mode=pad_mode)
    try:
        ctx.set_option("v3", 2)
        D = L.stft(y, n_fft=2048, hop_length=hop, center=center, pad_mode=pad_mode)
        assert D.shape == ref.shape and _stft_close(D, ref)
        for power in (1.0, 2.0, 1.5):
            S, _ = L._spectrogram(y=y, n_fft=2048, hop_length=hop, power=power, center=center, pad_mode=pad_mode)
            assert np.all(np.abs(S - np.abs(ref) ** power) <= 4e-6 * (np.abs(ref) ** power).max())
        Dp = L.stft(torch.from_numpy(y).to("cuda:0"), n_fft=2048, hop_length=hop, center=center, pad_mode=pad_mode, row_align=128)
        assert Dp.stride(-1) == 1040 and _stft_close(Dp.cpu().numpy(), ref)
        ctx.set_option("v3", 0)
        D0 = L.stft(y, n_fft=2048, hop_length=hop, center=center, pad_mode=pad_mode)
        assert np.abs(D - D0).max() <= 1e-6 * np.abs(D0).max()
    finally:
        ctx.set_option("v3", 1)  # (the library's default: complex epilogue only)


def test_radix_16_16_4_forward_full_size(L, full_batch):
    """BASELINE configs[3]'s forward leg through variant 6: 256 x 30 s, sampled clips against the oracle, round trip through the inverse kernel >= 60 dB on every clip."""
    import torch
    ctx = L.get_context(0)
    yt = full_batch
    try:
        ctx.set_option("v3", 1)
        D = L.stft(yt, n_fft=2048, hop_length=512)
        for i in (0, 100, 255):
            assert _stft_close(D[i].cpu().numpy(), O.stft(yt[i].cpu().numpy(), n_fft=2048, hop_length=512))
        yh = L.istft(D, hop_length=512, length=yt.shape[-1])
        err = ((yt - yh).double() ** 2).sum(-1)
        snr = 10 * torch.log10((yt.double() ** 2).sum(-1) / err)
        assert float(snr.min()) >= 60.0
    finally:
        ctx.set_option("v3", 1)


# ---- phase vocoder / time stretch (librosa/core/spectrum.py:1364-1519, effects.py:404-484) -------------
def _pv_close(a, ref):
    tol = 1e-11 if a.dtype == np.complex128 else 3e-5
    return a.shape == ref.shape and a.dtype == ref.dtype and np.all(np.abs(a - ref) <= tol * np.abs(ref) + tol * np.abs(ref).max())


def test_phase_vocoder_and_time_stretch_golden(L):
    import torch

    g = np.load(os.path.join(GOLDEN_DIR, "vocoder.npz"))
    D = g["D"]
    assert _pv_close(L.phase_vocoder(D, rate=2.0), g["pv_rate2"])
    assert _pv_close(L.phase_vocoder(D, rate=0.6), g["pv_rate06"])
    assert _pv_close(L.phase_vocoder(D, t_out=g["t_out"]), g["pv_tout"])
    assert _pv_close(L.phase_vocoder(g["D64"], rate=0.8), g["pv64_rate08"])
    assert _pv_close(L.phase_vocoder(np.ascontiguousarray(D), rate=1.0), O.phase_vocoder(D, rate=1.0))
    Dt = torch.from_numpy(np.ascontiguousarray(D)).cuda()
    out = L.phase_vocoder(Dt, rate=0.6)
    assert isinstance(out, torch.Tensor) and out.is_cuda and np.array_equal(out.cpu().numpy(), L.phase_vocoder(D, rate=0.6))
    with pytest.warns(FutureWarning, match="deprecated"):
        ts = L.effects.time_stretch(g["y"], rate=1.5, n_fft=1024, hop_length=256)
    ref = g["ts_15"]
    assert ts.shape == ref.shape and ts.dtype == ref.dtype and np.abs(ts - ref).max() <= 5e-5 * np.abs(ref).max()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        ts2 = L.effects.time_stretch(g["ys"], rate=0.7)
        ref2 = g["ts_stereo_07_default"]
        assert ts2.shape == ref2.shape and np.abs(ts2 - ref2).max() <= 5e-5 * np.abs(ref2).max()
        tsd = L.effects.time_stretch(torch.from_numpy(g["ys"]).cuda(), rate=0.7)
        assert isinstance(tsd, torch.Tensor) and np.array_equal(tsd.cpu().numpy(), ts2)
    for bad in (dict(), dict(rate=1.0, t_out=np.arange(3.0)), dict(rate=-1), dict(t_out=np.array([0.0, 47.0])), dict(rate=2.0, kind="cubic")):
        with pytest.raises(L.ParameterError):
            L.phase_vocoder(D, **bad)
    with pytest.raises(L.ParameterError):
        L.effects.time_stretch(g["y"], rate=0)


def test_device_resident_mask_round_trip(L):
    """effects.hpss-shaped use (librosa/effects.py:161-185): stft -> mask -> istft with the spectra never leaving the device,
    against the same chain through the oracle."""
    import torch

    y = golden_cases.make_signal("mix", 30000, 71, (2,), "float32")
    D = L.stft(torch.from_numpy(y).cuda(), n_fft=1024)
    mag = D.abs()
    mask = (mag > mag.mean(dim=-1, keepdim=True)).to(D.dtype)   # a "harmonic / percussive"-style binary mask, computed on the device
    yh = L.istft(D * mask, length=y.shape[-1])
    assert isinstance(yh, torch.Tensor) and yh.is_cuda
    Dr = O.stft(y, n_fft=1024)
    mr = (np.abs(Dr) > np.abs(Dr).mean(axis=-1, keepdims=True)).astype(Dr.dtype)
    # a bin whose magnitude sits within rounding of its row mean may flip sides: compare where the two masks agree
    same = np.array_equal(mr, mask.cpu().numpy())
    ref = O.istft(Dr * (mask.cpu().numpy() if not same else mr), length=y.shape[-1])
    assert np.abs(yh.cpu().numpy() - ref).max() <= 2e-5 * np.abs(ref).max()


@pytest.mark.parametrize("n_fft,hop,center,pad_mode", [(8192, 512, True, "constant"), (8192, 4096, True, "reflect"), (8192, 1024, False, "constant"), (16384, 1024, True, "edge"), (16384, 8192, True, "symmetric")])
def test_register_ring_large_frames(L, n_fft, hop, center, pad_mode):
    """n_fft >= 8192 with hop = n_fft / {2, 4, 8, 16} (BASELINE configs[4]'s n_fft = 8192 leg): the sample ring lives in
    registers (stft_kernel<..., RA = 3 .. 6>); with the option off the LDS-ring kernels must give the same numbers."""
    ctx = L.get_context(0)
    rng = np.random.default_rng(n_fft + hop)
    y = rng.standard_normal((3, 90001)).astype(np.float32)
    ref = O.stft(y, n_fft=n_fft, hop_length=hop, center=center, pad_mode=pad_mode)
    try:
        D = L.stft(y, n_fft=n_fft, hop_length=hop, center=center, pad_mode=pad_mode)
        assert D.shape == ref.shape and _stft_close(D, ref)
        S, _ = L._spectrogram(y=y, n_fft=n_fft, hop_length=hop, power=1, center=center, pad_mode=pad_mode)
        assert np.all(np.abs(S - np.abs(ref)) <= 4e-6 * np.abs(ref).max())
        ctx.set_option("direct", 0)
        assert _stft_close(L.stft(y, n_fft=n_fft, hop_length=hop, center=center, pad_mode=pad_mode), ref)
    finally:
        ctx.set_option("direct", 1)


@pytest.mark.parametrize("n_fft,hop", [(8192, 512), (2048, 128), (4096, 256), (16384, 1024), (256, 16)])
def test_istft_sixteenth_hop(L, n_fft, hop):
    """hop = n_fft / 16 takes the row-aligned overlap-add with one row per hop (n_fft = 8192 at hop 512 is the inverse of
    BASELINE configs[4]'s widest leg); round trip and oracle comparison, with and without `length`."""
    rng = np.random.default_rng(n_fft + hop)
    y = rng.standard_normal((2, 100003)).astype(np.float32)
    D = O.stft(y, n_fft=n_fft, hop_length=hop)
    for length in (None, y.shape[-1], 90000):
        ref = O.istft(D, hop_length=hop, length=length)
        got = L.istft(D, hop_length=hop, length=length)
        wss = _wss_for(dict(n_fft=n_fft, hop_length=hop), D.shape[-1], ref.shape[-1], length, np.float32)
        assert got.shape == ref.shape and _istft_close(got, ref, wss)
    assert np.abs(L.istft(D, hop_length=hop, length=y.shape[-1]) - y).max() <= 2e-5


@pytest.mark.parametrize("clips", [1, 2])
def test_istft_ascending_radix_general_hop(L, clips):
    """Context option variant = 5 pins the inverse to the ascending-radix configuration (radices 8, 8, 16); with a hop that is no whole number of
    rows it runs the general overlap-add mode there (istft_kernel<cfg_f32_10r, 0>, csrc/lra_fused.h instance group 13), which no default call
    reaches.  3 n_fft + 1 samples against the oracle with the inverse's bar."""
    n_fft, hop = 2048, 300
    ctx = L.get_context(0)
    y = np.random.default_rng(n_fft + hop + clips).standard_normal((clips, 3 * n_fft + 1)).astype(np.float32)
    D = O.stft(y, n_fft=n_fft, hop_length=hop)
    ref = O.istft(D, hop_length=hop)
    wss = _wss_for(dict(n_fft=n_fft, hop_length=hop), D.shape[-1], ref.shape[-1], None, np.float32)
    try:
        ctx.set_option("variant", 5)
        got = L.istft(D, hop_length=hop)
    finally:
        ctx.set_option("variant", -1)
    assert got.shape == ref.shape and _istft_close(got, ref, wss)


@pytest.mark.parametrize(
    "n_fft,hop,center,n,lengths,dtype",
    [
        (2048, 512, True, 50000, (None, 50000, 40000, 60000, 70001), np.float32),   # the BASELINE shape: register carry, rows of HC = R/4
        (2048, 512, False, 50000, (None, 48000, 53000), np.float32),
        (2048, 1024, True, 30000, (None, 30000, 40000), np.float32),
        (2048, 128, True, 20000, (None, 25000), np.float32),
        (2048, 441, True, 30000, (None, 30000, 36000), np.float32),                 # general overlap-add of the fused kernel
        (1024, 256, True, 30000, (None, 33000), np.float32),                        # two slots per wave
        (512, 512, True, 9000, (None, 9000, 11000), np.float32),                    # hop == n_fft: no carry
        (256, 300, True, 5000, (None, 5000, 7000), np.float32),                     # hop > n_fft: gaps between frames
        (256, 300, False, 5000, (None, 6500), np.float32),
        (8192, 512, True, 60000, (None, 70000), np.float32),                        # four waves per frame
        (1000, 250, True, 20000, (None, 20000, 26000), np.float32),                 # mixed-radix fused inverse (4 x 5 x 5 x 5)
        (400, 160, True, 30000, (None, 30000, 36000), np.float32),                  # ... 8 x 5 x 5: several groups per clip, halo frames
        (400, 160, False, 30000, (None, 33000), np.float64),
        (160, 200, True, 9000, (None, 12000), np.float32),                          # ... hop > n_fft
        (512, 200, True, 30000, (None, 30000, 36000), np.float32),                  # ... powers of two with a hop outside n_fft / {2, 4, 8, 16}: the same gather kernel
        (256, 100, False, 20000, (None, 23000), np.float64),
        (256, 80, True, 20000, (None, 20000), np.float32),
        (512, 160, True, 30000, (None, 33000), np.float32),                         # (own frames < 2 x halo: stays with the register-tiled kernel's general mode)
        (1002, 250, True, 20000, (None, 20000, 26000), np.float32),                 # rocFFT + gather path (n_fft / 2 = 501 = 3 x 167)
        (2048, 512, True, 30000, (None, 36000), np.float64),
    ],
)
def test_istft_stores_every_sample(L, n_fft, hop, center, n, lengths, dtype):
    """The inverse kernels write every output sample themselves; the host wrapper zeroes only what no frame reaches (`length` beyond the
    frames: core/spectrum.py:553-555, 606-624).  Outputs are allocated full of NaN bit patterns here, so a sample nobody stores fails
    the comparison with the oracle.  (Round 3 cleared the whole output ahead of every launch: 10.7 % of the call.)"""
    import torch

    from librosa_amd import _arrays

    rng = np.random.default_rng(n_fft * 7 + hop)
    y = rng.standard_normal((3, n)).astype(dtype)
    D = O.stft(y, n_fft=n_fft, hop_length=hop, center=center)
    Dt = torch.from_numpy(D).cuda()
    old = _arrays.POISON_OUTPUTS
    _arrays.POISON_OUTPUTS = True
    try:
        for length in lengths:
            ref = O.istft(D, hop_length=hop, n_fft=n_fft, center=center, length=length)
            wss = _wss_for(dict(n_fft=n_fft, hop_length=hop, center=center), D.shape[-1], ref.shape[-1], length, dtype)
            got = L.istft(Dt, hop_length=hop, n_fft=n_fft, center=center, length=length).cpu().numpy()
            assert got.shape == ref.shape
            assert np.isfinite(got).all(), (length, int(np.isnan(got).sum()), np.flatnonzero(np.isnan(got[0]))[:4])
            assert _istft_close(got, ref, wss), length
            got_np = L.istft(D, hop_length=hop, n_fft=n_fft, center=center, length=length)   # NumPy path: host pipeline, its own device buffers
            assert np.isfinite(got_np).all() and _istft_close(got_np, ref, wss), length
    finally:
        _arrays.POISON_OUTPUTS = old


def test_numpy_batch_shards_in_process(L, monkeypatch):
    """a NumPy batch is split into contiguous clip ranges, one per device named by LRA_DEVICES, each through that device's
    own context and host pipeline.  A 1-GPU box runs the degenerate case -- both ranges on device 0 -- which exercises the range / pointer /
    stride arithmetic of stft (incl. out=), _spectrogram, melspectrogram and istft; the result must equal the unsharded call bit for bit
    (the reference's batch == per item property, tests/test_multichannel.py:96-111)."""
    from librosa_amd.core import spectrum

    y = golden_cases.make_signal("noise", 30000, 11, (5,))
    monkeypatch.setenv("LRA_DEVICES", "0")
    D1 = L.stft(y, n_fft=1024, hop_length=256)
    M1 = L.feature.melspectrogram(y=y, sr=22050, n_fft=1024, hop_length=256, n_mels=40)
    S1, _ = spectrum._spectrogram(y=y, n_fft=1024, hop_length=256, power=2)
    y1 = L.istft(D1, hop_length=256, length=y.shape[-1])
    monkeypatch.setattr(spectrum, "_MULTI_DEVICE_MIN_BYTES", 0)
    n_dev = L.device_count()
    monkeypatch.setenv("LRA_DEVICES", ",".join(str(i % n_dev) for i in range(2)) if n_dev < 2 else "all")
    served = []
    orig = spectrum._sharded_host_exec

    def spy(sess, batch, nbytes, run):
        return orig(sess, batch, nbytes, lambda c, b, e: (served.append((c.device, b, e)), run(c, b, e))[1])

    monkeypatch.setattr(spectrum, "_sharded_host_exec", spy)
    D2 = L.stft(y, n_fft=1024, hop_length=256)
    assert len(served) >= 2 and sorted((b, e) for _, b, e in served)[0][0] == 0 and sum(e - b for _, b, e in served) == 5
    assert np.array_equal(D1, D2)
    assert np.array_equal(M1, L.feature.melspectrogram(y=y, sr=22050, n_fft=1024, hop_length=256, n_mels=40))
    assert np.array_equal(S1, spectrum._spectrogram(y=y, n_fft=1024, hop_length=256, power=2)[0])
    assert np.array_equal(y1, L.istft(D2, hop_length=256, length=y.shape[-1]))
    out = np.swapaxes(np.zeros((5, D1.shape[-1] + 3, 513), dtype=np.complex64), -1, -2)   # laid out like stft's own result, three spare columns
    got = L.stft(y, n_fft=1024, hop_length=256, out=out)
    assert np.array_equal(got, D1) and np.shares_memory(got, out)
    # three ranges of unequal length (7 clips -> 3 + 2 + 2), all on device 0
    y7 = golden_cases.make_signal("noise", 20000, 12, (7,))
    monkeypatch.setenv("LRA_DEVICES", "0")
    M7 = L.feature.melspectrogram(y=y7, sr=22050, n_fft=1024, hop_length=256, n_mels=40)
    monkeypatch.setenv("LRA_DEVICES", "0,0,0")
    del served[:]
    assert np.array_equal(M7, L.feature.melspectrogram(y=y7, sr=22050, n_fft=1024, hop_length=256, n_mels=40))
    assert sorted(e - b for _, b, e in served) == [2, 2, 3]
    monkeypatch.setenv("LRA_DEVICES", ",".join(str(i % n_dev) for i in range(2)) if n_dev < 2 else "all")
    bad = y.copy()
    bad[4, 17] = np.nan   # a non-finite sample in the LAST range must still raise
    with pytest.raises(L.ParameterError):
        L.stft(bad, n_fft=1024, hop_length=256)


@pytest.mark.parametrize("n_fft,hop,sr,n_mels", [(256, 64, 8000, 80), (256, 100, 8000, 56), (128, 32, 8000, 64), (128, 50, 8000, 40)])
def test_small_pow2_mel_many_bands_flat_index(L, n_fft, hop, sr, n_mels):
    """Round 6: the fused mel at n_fft 128 / 256 with many bands (from 40 / 56) runs the flat-index kernel of csrc/lra_mixed.h instead of the register-tiled one (whose
    8- and 4-thread frames leave the band combine to too few lanes: 256 / 64 / 80 bands 2.02 -> 1.28 ms over 256 x 30 s); both against the oracle at the usual bars, every
    pad mode, float64, and each other (ctx option mixed_pow2_mel).  Reference: feature/spectral.py:2022-2161."""
    rng = np.random.default_rng(n_fft + hop)
    y = (0.1 * rng.standard_normal((3, 40 * n_fft + 11))).astype(np.float32)
    ctx = L.get_context(0)
    outs = {}
    try:
        for opt in (1, 0):
            ctx.set_option("mixed_pow2_mel", opt)
            for center, pad_mode in ((True, "constant"), (True, "reflect"), (False, "constant")):
                Mref = O.melspectrogram(y=y, sr=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels, center=center, pad_mode=pad_mode)
                M = L.feature.melspectrogram(y=y, sr=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels, center=center, pad_mode=pad_mode)
                assert M.shape == Mref.shape and _mel_close(M, Mref), (opt, center, pad_mode)
                assert np.all(np.abs(M - Mref) <= 1e-4 * np.abs(Mref) + 1e-7 * Mref.max())
                outs[(opt, center, pad_mode)] = M
            y64 = y[:2].astype(np.float64)
            assert _mel_close(L.feature.melspectrogram(y=y64, sr=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels), O.melspectrogram(y=y64, sr=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels))
            S1 = L.feature.melspectrogram(y=y, sr=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels, power=1.0)
            assert _mel_close(S1, O.melspectrogram(y=y, sr=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels, power=1.0))
    finally:
        ctx.set_option("mixed_pow2_mel", 1)
    # (the stft / |X|^p of these sizes stay on the register-tiled kernels either way)
    assert _stft_close(L.stft(y, n_fft=n_fft, hop_length=hop), O.stft(y, n_fft=n_fft, hop_length=hop))


@pytest.mark.parametrize("n_fft,hop,sr,n_mels", [(400, 160, 16000, 80), (320, 160, 16000, 40), (480, 120, 48000, 64), (800, 200, 16000, 128), (960, 480, 48000, 80),
                                                 (1200, 300, 48000, 128), (1600, 400, 16000, 80), (2400, 600, 48000, 128), (240, 80, 8000, 20), (4800, 1200, 48000, 128),
                                                 (882, 441, 44100, 64), (1764, 441, 44100, 128), (2646, 882, 44100, 128), (3528, 882, 44100, 128), (600, 240, 24000, 80), (720, 180, 48000, 64)])
def test_mixed_radix_frames_fused(L, n_fft, hop, sr, n_mels):
    """Frame lengths 2^a 3^b 5^c (400 / 160 = the 25 ms / 10 ms front end of 16 kHz speech models; reference sizes: tests/test_core.py:256-292) run ONE fused
    launch (csrc/lra_mixed.h) instead of framing + rocFFT + transpose + banded product: stft, |X|^p and melspectrogram against the oracle, the pad modes,
    float64, device tensors, and agreement with the rocFFT path they replace (ctx option "mixed")."""
    import torch

    rng = np.random.default_rng(n_fft + hop)
    y = (0.1 * rng.standard_normal((3, 11 * n_fft + 17))).astype(np.float32)
    ctx = L.get_context(0)
    for center, pad_mode in ((True, "constant"), (True, "reflect"), (False, "constant")):
        ref = O.stft(y, n_fft=n_fft, hop_length=hop, center=center, pad_mode=pad_mode)
        D = L.stft(y, n_fft=n_fft, hop_length=hop, center=center, pad_mode=pad_mode)
        assert D.shape == ref.shape and D.dtype == ref.dtype and _stft_close(D, ref), (center, pad_mode)
    Mref = O.melspectrogram(y=y, sr=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels)
    M = L.feature.melspectrogram(y=y, sr=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels)
    assert M.shape == Mref.shape and _mel_close(M, Mref)
    assert np.all(np.abs(M - Mref) <= 1e-4 * np.abs(Mref) + 1e-7 * Mref.max())
    Mt = L.feature.melspectrogram(y=torch.from_numpy(y).cuda(), sr=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels).cpu().numpy()
    assert np.array_equal(Mt, M)
    S1 = L.feature.melspectrogram(y=y, sr=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels, power=1.0)
    assert _mel_close(S1, O.melspectrogram(y=y, sr=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels, power=1.0))
    y64 = y[:2].astype(np.float64)
    assert _stft_close(L.stft(y64, n_fft=n_fft, hop_length=hop), O.stft(y64, n_fft=n_fft, hop_length=hop))
    assert _mel_close(L.feature.melspectrogram(y=y64, sr=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels), O.melspectrogram(y=y64, sr=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels))
    # the path it replaces, same inputs: both must satisfy the oracle, and each other to the same tolerance
    try:
        ctx.set_option("mixed", 0)
        D0 = L.stft(y, n_fft=n_fft, hop_length=hop)
        M0 = L.feature.melspectrogram(y=y, sr=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels)
    finally:
        ctx.set_option("mixed", 1)
    assert _stft_close(L.stft(y, n_fft=n_fft, hop_length=hop), D0) and _mel_close(M, M0)
    # the fused inverse of the same frame lengths: round trip, the oracle with and without `length`, and the rocFFT path it replaces
    Dfull = L.stft(y, n_fft=n_fft, hop_length=hop)
    yh = L.istft(Dfull, hop_length=hop, n_fft=n_fft, length=y.shape[-1])
    assert np.abs(yh - y).max() <= 2e-5
    Dref = O.stft(y, n_fft=n_fft, hop_length=hop)
    for length in (None, y.shape[-1], y.shape[-1] - 3 * hop - 1, y.shape[-1] + 2 * n_fft):
        ref = O.istft(Dref, hop_length=hop, n_fft=n_fft, length=length)
        got = L.istft(Dref, hop_length=hop, n_fft=n_fft, length=length)
        wss = _wss_for(dict(n_fft=n_fft, hop_length=hop), Dref.shape[-1], ref.shape[-1], length, np.float32)
        assert got.shape == ref.shape and _istft_close(got, ref, wss), length
    try:
        ctx.set_option("mixed", 0)
        y0 = L.istft(Dfull, hop_length=hop, n_fft=n_fft, length=y.shape[-1])
    finally:
        ctx.set_option("mixed", 1)
    assert np.abs(y0 - yh).max() <= 2e-6 * max(1.0, np.abs(y).max())


def test_bench_two_ranks_with_real_kernels():
    """the N > 1 path of bench.py with REAL kernels -- two ranks (gloo for the rendezvous / barriers / gather, both on device 0 of the
    1-GPU box, which bench.py allows under LRA_BENCH_BACKEND=gloo), configs[2]'s split shape at a smaller per-rank batch: one JSON line with n_gpus = 2,
    the chunked gather's own rows AND the neighbour's rows equal to the unsharded computation."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LRA_DEVICES")}
    env.update(LRA_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "48", "--prewarm-ms", "50", "--gather-chunks", "3", "--full"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert len(lines[0]) <= 4096
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["value"] > 0 and line["config"]["clips_per_gpu"] == 48
    g = line["gathered"]
    assert g["own_rows_match"] is True and g["full_matches_unsharded"] is True and g["backend"] == "gloo" and g["chunks"] == 3


def test_native_rccl_communicator(L):
    """lra_comm_* (RCCL bound at run time through the C ABI) at world size 1 -- all a one-GPU box can run: id, communicator on
    the context's device, an all-gather enqueued behind the kernel that produced its input."""
    import torch

    from librosa_amd import _native
    from librosa_amd.distributed import NativeGather

    uid = _native.comm_unique_id()
    assert len(uid) == _native.COMM_ID_BYTES and any(uid)
    ctx = L.get_context(0)
    g = NativeGather(ctx, 0, 1, uid)
    y = torch.from_numpy(O.config_input(3, n=22050)).cuda()
    M = L.feature.melspectrogram(y=y, sr=22050)
    full = g.all_gather(M)
    torch.cuda.synchronize()
    assert full.shape == M.shape and torch.equal(full, M)
    assert torch.equal(g.all_gather(M, n_items=3), M)
    with pytest.raises(ValueError):
        g.all_gather(M, n_items=5)  # this rank would hold 5 items, not 3
    # the unequal-shard form (one grouped broadcast per rank into its slice), as far as one rank can exercise it: its piece lands at the given offset
    big = torch.full((5,) + tuple(M.shape[1:]), float("nan"), device=M.device)
    row = M[0].numel() * M.element_size()
    g.comm.allgatherv(M.data_ptr(), big.data_ptr(), [3 * row], [2 * row])
    torch.cuda.synchronize()
    assert torch.equal(big[2:], M) and bool(torch.isnan(big[:2]).all())
    g.close()
    with pytest.raises(L.ParameterError):
        _native.Comm(ctx, 2, 1, uid)  # rank outside the world


# ---- PCEN (librosa/core/spectrum.py:2396-2666, docs/examples/plot_pcen_stream.py:71-80) -----------------------
# The reference computes PCEN in float64 for every input type; the device does too.  The smoother recurrence is the same
# sequence of IEEE operations (the filter state is compared to 1e-15); the elementwise part goes through exp / log1p / expm1 /
# log, where device and host libm differ in the last bits: 1e-11 relative.  bias == 0 takes log(S) in S's own precision
# (float32 for float32 input, NumPy's SIMD loop): 1e-5 relative there.
def _pcen_close(got, ref, tol=1e-11):
    return got.shape == ref.shape and got.dtype == ref.dtype and np.all(np.abs(got - ref) <= tol * np.abs(ref))


def test_pcen_golden(L):
    import torch

    g = np.load(os.path.join(GOLDEN_DIR, "pcen.npz"))
    inputs = golden_cases.pcen_inputs(g)
    for name, (key, kw) in golden_cases.PCEN_CASES.items():
        tol = 1e-5 if (kw.get("bias", 2) == 0 and inputs[key].dtype == np.float32) else 1e-11
        got = L.pcen(inputs[key], **kw)
        assert _pcen_close(got, g[name], tol), (name, np.max(np.abs(got - g[name]) / np.abs(g[name]).clip(1e-300)))
        dev = L.pcen(torch.from_numpy(inputs[key]).cuda(), **kw)
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float64 and np.array_equal(dev.cpu().numpy(), got), name
    assert _pcen_close(L.pcen(g["A"], ref=g["ref_in"]), g["with_ref"])
    # two blocks with the carried filter state (the streaming example), NumPy and device-resident
    p1, z1 = L.pcen(g["A"][:, :25], return_zf=True)
    p2, z2 = L.pcen(g["A"][:, 25:], zi=z1, return_zf=True)
    for got, key in ((p1, "block1"), (p2, "block2")):
        assert _pcen_close(got, g[key]), key
    for got, key in ((z1, "zf1"), (z2, "zf2")):
        assert _pcen_close(got, g[key], 1e-15), key
    At = torch.from_numpy(g["A"]).cuda()
    q1, y1 = L.pcen(At[:, :25], return_zf=True)
    q2, y2 = L.pcen(At[:, 25:], zi=y1, return_zf=True)
    assert y1.is_cuda and np.array_equal(q2.cpu().numpy(), p2) and np.array_equal(y2.cpu().numpy(), z2)
    q2b = L.pcen(At[:, 25:], zi=z1)                               # host state, device data
    assert np.array_equal(q2b.cpu().numpy(), p2)


def test_pcen_reference_test_matrix(L):
    """The reference's own PCEN tests (tests/test_core.py:2354-2573) against the device path."""
    rng = np.random.default_rng(628318)
    S = np.abs(rng.standard_normal((9, 30)))
    for kw in (dict(gain=-1), dict(bias=-1), dict(power=-0.1), dict(b=-2), dict(b=2), dict(time_constant=-2), dict(eps=0), dict(max_size=1.5), dict(max_size=0)):
        with pytest.raises(L.ParameterError):
            L.pcen(S, **{**dict(gain=1, bias=1, power=1, b=0.5, time_constant=0.5, eps=1e-6, max_size=1), **kw})
    for p in (0.5, 1, 2):   # b=1, gain=0, bias=0: all filtering disabled
        assert np.allclose(L.pcen(S, gain=0, bias=0, power=p, b=1, time_constant=0.5, eps=1e-6, max_size=1), S**p)
    assert np.allclose(L.pcen(S, gain=1, bias=0, power=1, b=1, time_constant=0.5, eps=1e-20, max_size=1), np.ones_like(S))
    for power in (0, 1e-3):
        for bias in (0, 1):
            P = L.pcen(S, gain=0.0, bias=bias, power=power, eps=1e-20)
            back = np.expm1(P) if power == 0 else (np.exp(1.0 / power * np.log(P)) if bias == 0 else np.expm1(1.0 / power * np.log1p(P)))
            assert np.allclose(S, back)
    with pytest.warns(UserWarning, match="complex"):
        P = L.pcen(np.ones((9, 30), dtype=complex), gain=1, bias=0, power=1, time_constant=0.5, eps=1e-20, b=1, max_size=1)
    assert P.shape == (9, 30) and np.allclose(P, 1)
    for max_size in (1, 3):
        assert np.allclose(L.pcen(np.zeros((9, 30)), gain=0.98, bias=2.0, power=0.5, b=None, time_constant=0.395, eps=1e-6, max_size=max_size), 0)
    X = rng.standard_normal((3, 100, 50)) ** 2
    for ms in (1, 3):
        P1 = L.pcen(X[0], max_size=ms)
        assert _pcen_close(P1, O.pcen(X[0], max_size=ms))
        assert np.array_equal(P1, L.pcen(X[0], axis=-1, max_size=ms)) and np.array_equal(P1, L.pcen(X[0].T, axis=0, max_size=ms).T)
    Pa = L.pcen(X)
    Pm = L.pcen(X, max_size=3, max_axis=1)
    for i in range(3):
        assert np.array_equal(L.pcen(X[i]), Pa[i]) and np.array_equal(L.pcen(X[i], max_size=3), Pm[i])
    with pytest.raises(L.ParameterError):
        L.pcen(X, max_size=3)                      # 3-d input needs max_axis
    with pytest.raises(L.ParameterError):
        L.pcen(np.arange(100), max_size=3)         # no max filter over a 1-d input
    X2 = rng.standard_normal((100, 50)) ** 2
    assert np.allclose(L.pcen(X2, gain=1, bias=0, power=1, b=1, ref=np.ones_like(X2), eps=1e-20), X2)
    for x in (np.arange(100), np.arange(100).reshape((10, 10))):     # integer input, 1-d and 2-d, split in two blocks
        x1, x2 = x[..., :20], x[..., 20:]
        p1, zf1 = L.pcen(x1, return_zf=True)
        p2, _ = L.pcen(x2, zi=zf1, return_zf=True)
        full = L.pcen(x)
        assert np.allclose(full, np.hstack([p1, p2])) and _pcen_close(full, O.pcen(x))
    x = rng.standard_normal((20, 50, 60)) ** 2
    for axis in (0, 1, 2, -2, -1):
        s1, s2 = [slice(None)] * 3, [slice(None)] * 3
        s1[axis], s2[axis] = slice(0, 10), slice(10, None)
        p1, zf1 = L.pcen(x[tuple(s1)], return_zf=True, axis=axis)
        p2, _ = L.pcen(x[tuple(s2)], zi=zf1, return_zf=True, axis=axis)
        full = L.pcen(x, axis=axis)
        assert np.allclose(full, np.concatenate([p1, p2], axis=axis), rtol=1e-12, atol=0) and _pcen_close(full, O.pcen(x, axis=axis))
        assert zf1.shape == tuple(1 if a == axis % 3 else x[tuple(s1)].shape[a] for a in range(3))


def test_pcen_streaming_example(L):
    """docs/examples/plot_pcen_stream.py:62-80: stream -> stft(center=False, out=D) -> pcen(|D|, zi=zi, return_zf=True), block by block,
    against the oracle's PCEN with the same carried state and against one PCEN pass over all frames."""
    n_fft, hop, block_length, sr = 2048, 512, 16, 22050
    y = O.config_input(1, n=sr * 4)[0]
    D, zi, zo, got, exp, mags = None, None, None, [], [], []
    for blk in L.stream(y, block_length=block_length, frame_length=n_fft, hop_length=hop):
        D = L.stft(blk, n_fft=n_fft, hop_length=hop, center=False, out=D)
        mag = np.abs(D)
        mags.append(mag)
        P, zi = L.pcen(mag, sr=sr, hop_length=hop, zi=zi, return_zf=True)
        got.append(P)
        # the oracle on the SAME magnitudes (the block STFTs have their own parity tests; PCEN's gain control would amplify their
        # float32 noise floor in quiet bins)
        Po, zo = O.pcen(mag, sr=sr, hop_length=hop, zi=zo, return_zf=True)
        exp.append(Po)
        assert _pcen_close(zi, zo, 1e-15)
    got, exp = np.concatenate(got, axis=-1), np.concatenate(exp, axis=-1)
    assert _pcen_close(got, exp)
    n_whole = 1 + (len(y) - n_fft) // hop
    assert got.shape == (1025, n_whole)
    whole = L.pcen(np.concatenate(mags, axis=-1), sr=sr, hop_length=hop)      # one pass over all frames == block by block with the carried state
    assert np.array_equal(got, whole)


def test_pcen_full_size_properties(L):
    """BASELINE configs[1] shape: the mel spectrograms of 256 clips x 30 s (256 x 128 x 1292 float32), device-resident.  Sampled rows
    against the oracle; two blocks with the carried state == one pass; max-filtered variant against the oracle on one clip."""
    import torch

    torch.manual_seed(5)
    M = torch.rand((256, 128, 1292), device="cuda", dtype=torch.float32) ** 4 * 50.0
    P = L.pcen(M)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    P = L.pcen(M)
    ev1.record()
    torch.cuda.synchronize()
    print(f"pcen 256x128x1292 f32 -> f64: {ev0.elapsed_time(ev1):.3f} ms")
    assert P.shape == M.shape and P.dtype == torch.float64
    for clip in (0, 131, 255):
        assert _pcen_close(P[clip].cpu().numpy(), O.pcen(M[clip].cpu().numpy()))
    p1, zf = L.pcen(M[..., :700], return_zf=True)
    p2 = L.pcen(M[..., 700:], zi=zf)
    assert torch.equal(torch.cat([p1, p2], dim=-1), P)
    Pm = L.pcen(M[:2], max_size=3, max_axis=-2)
    assert _pcen_close(Pm[1].cpu().numpy(), O.pcen(M[1].cpu().numpy(), max_size=3))


# ---- constant-Q / variable-Q transform (librosa/core/constantq.py:42-225, 820-1122) -----------------------------
# float32: the octave STFTs carry the forward kernel's own error (~2e-7 of their peak), the projection sums up to a few hundred of
# their bins: 2e-5 of the transform's peak.  float64: 1e-11.  Between octaves the decimated signals are bit-identical to scipy's
# resample_poly (tests/test_hostsim.py; on the device: tests/test_resample_gpu.py, every kernel of the decimator and the halving chain), so nothing accumulates
# down the recursion.
def _cqt_close(C, ref):
    tol = 1e-11 if C.dtype == np.complex128 else 2e-5
    return C.shape == ref.shape and C.dtype == ref.dtype and np.abs(C - ref).max() <= tol * np.abs(ref).max()


@pytest.mark.parametrize("name", list(golden_cases.CQT_CASES))
def test_cqt_golden(L, name):
    import torch

    fn, (kind, n, seed, channels, dtype), kw = golden_cases.CQT_CASES[name]
    g = np.load(os.path.join(GOLDEN_DIR, "cqt.npz"))
    y = golden_cases.make_signal(kind, n, seed, channels, dtype)
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message="n_fft=.*is too large")
        C = getattr(L, fn)(y, sr=golden_cases.SR, res_type="polyphase", **kw)
        assert _cqt_close(C, g[name]), np.abs(C - g[name]).max() / np.abs(g[name]).max()
        Ct = getattr(L, fn)(torch.from_numpy(y).cuda(), sr=golden_cases.SR, res_type="polyphase", **kw)
    assert isinstance(Ct, torch.Tensor) and Ct.is_cuda and np.array_equal(Ct.cpu().numpy(), C)


@pytest.mark.parametrize("name", list(golden_cases.CQT_FFT_CASES))
def test_cqt_fft_resampler_golden(L, name):
    """res_type="fft" / "scipy": the octaves are resampled by whole-signal transforms (lra_resample_fft_exec: rocFFT both ways) --
    against the unmodified reference's output.  float32 transforms of up to 33 075 points on both sides: 1e-4 of the peak."""
    import torch

    fn, (kind, n, seed, channels, dtype), kw = golden_cases.CQT_FFT_CASES[name]
    g = np.load(os.path.join(GOLDEN_DIR, "resample.npz"))
    y = golden_cases.make_signal(kind, n, seed, channels, dtype)
    tol = 1e-10 if dtype == "float64" else 1e-4
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message="n_fft=.*is too large")
        C = getattr(L, fn)(y, sr=golden_cases.SR, **kw)
        assert C.shape == g[name].shape and C.dtype == g[name].dtype and np.abs(C - g[name]).max() <= tol * np.abs(g[name]).max(), np.abs(C - g[name]).max() / np.abs(g[name]).max()
        Ct = getattr(L, fn)(torch.from_numpy(y).cuda(), sr=golden_cases.SR, **kw)
    assert isinstance(Ct, torch.Tensor) and Ct.is_cuda and np.array_equal(Ct.cpu().numpy(), C)


@pytest.mark.parametrize("name", list(golden_cases.RESAMPLE_CASES))
def test_resample_golden(L, name):
    """librosa_amd.resample against the unmodified reference (tests/golden/resample.npz): the Fourier converter to float32 / float64
    transform accuracy (1e-5 / 1e-12 of the peak), the polyphase converter bit for bit (scipy's taps, upfirdn's summation order)."""
    import torch

    (kind, n, seed, channels, dtype), kw = golden_cases.RESAMPLE_CASES[name]
    g = np.load(os.path.join(GOLDEN_DIR, "resample.npz"))
    y = golden_cases.make_signal(kind, n, seed, channels, dtype)
    got = L.resample(y, **kw)
    assert got.shape == g[name].shape and got.dtype == g[name].dtype
    if kw["res_type"] == "polyphase":
        assert np.array_equal(got, g[name])
    else:
        assert np.abs(got - g[name]).max() <= (1e-12 if dtype == "float64" else 1e-5) * np.abs(g[name]).max(), np.abs(got - g[name]).max() / np.abs(g[name]).max()
    dev = L.resample(torch.from_numpy(y).cuda(), **kw)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)


@pytest.mark.parametrize("name", list(golden_cases.PITCH_SHIFT_CASES))
def test_pitch_shift_golden(L, name):
    """effects.pitch_shift = time_stretch + resample + fix_length, device-resident, against the unmodified reference: 2e-5 of the peak
    (the phase vocoder's and the whole-signal transforms' float32 rounding); NumPy and tensor input give the same samples; polyphase
    cannot take the non-integer intermediate rate (the reference's error)."""
    import torch

    (kind, n, seed, channels, dtype), kw = golden_cases.PITCH_SHIFT_CASES[name]
    g = np.load(os.path.join(GOLDEN_DIR, "resample.npz"))
    y = golden_cases.make_signal(kind, n, seed, channels, dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = L.effects.pitch_shift(y, sr=golden_cases.SR, **kw)
        dev = L.effects.pitch_shift(torch.from_numpy(y).cuda(), sr=golden_cases.SR, **kw)
        own = L.effects.pitch_shift(y, sr=golden_cases.SR, **{**kw, "res_type": "soxr_hq"})
    assert got.shape == g[name].shape and got.dtype == g[name].dtype and np.abs(got - g[name]).max() <= 2e-5 * np.abs(g[name]).max(), np.abs(got - g[name]).max() / np.abs(g[name]).max()
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)
    assert np.array_equal(own, got)   # the band-limited names take the Fourier converter for a non-integer rate
    with pytest.raises(L.ParameterError):
        L.effects.pitch_shift(y, sr=golden_cases.SR, n_steps=1, res_type="polyphase")
    with pytest.raises(L.ParameterError):
        L.effects.pitch_shift(y, sr=golden_cases.SR, n_steps=1, bins_per_octave=0)


@pytest.mark.parametrize("orig,target,n,dtype", [(22050, 16000, 9000, "float32"), (16000, 22050, 7001, "float32"), (44100, 48000, 5000, "float64"), (3, 2, 4096, "float32")])
def test_resample_band_limited_converter(L, orig, target, n, dtype):
    """The library's own converter for the soxr / kaiser / sinc names at a ratio that is not a plain decimation (lra_resample_band_exec:
    zero-padded clip, rfft, erfc roll-off at soxr-HQ's band edges, irfft on the exact output grid) against the same arithmetic in NumPy
    float64 -- and, being a linear convolution with a zero-phase low-pass, against scipy's polyphase converter on a band-limited signal."""
    import scipy.special
    from librosa_amd.core.audio import _band_plan

    rng = np.random.default_rng(n)
    y = rng.standard_normal((3, n)).astype(dtype)
    g = np.gcd(orig, target)
    up, down = target // g, orig // g
    got = L.resample(y, orig_sr=orig, target_sr=target, res_type="soxr_hq")
    fft_in, fft_out, k_mid, k_sigma = _band_plan(n, up, down)
    X = np.fft.rfft(y.astype(np.float64), n=fft_in, axis=-1)
    n_copy = min(fft_in, fft_out) // 2 + 1
    Y = np.zeros((3, fft_out // 2 + 1), dtype=np.complex128)
    Y[:, :n_copy] = X[:, :n_copy] * (0.5 * scipy.special.erfc((np.arange(n_copy) - k_mid) / k_sigma))
    exp = (np.fft.irfft(Y, n=fft_out, axis=-1) * (fft_out / fft_in))[:, : -(-n * up // down)]
    assert got.shape == exp.shape and got.dtype == y.dtype
    assert np.abs(got - exp).max() <= (1e-12 if dtype == "float64" else 2e-6) * np.abs(exp).max(), np.abs(got - exp).max() / np.abs(exp).max()
    t = np.arange(n)
    tone = (np.sin(0.11 * t) + 0.5 * np.cos(0.37 * t + 1.0)).astype(dtype) * np.hanning(n).astype(dtype)   # far below both band edges
    a = L.resample(tone, orig_sr=orig, target_sr=target, res_type="kaiser_best")
    b = L.resample(tone, orig_sr=orig, target_sr=target, res_type="polyphase")
    assert a.shape == b.shape and np.abs(a - b).max() <= 2e-3, np.abs(a - b).max()   # (Kaiser-5's own pass-band droop)


def test_magphase_reference_cases(L):
    """librosa.magphase (core/spectrum.py:1296-1361) on the device: the reference's own tests (tests/test_core.py:756-804: dtype propagation,
    zeros -> 1 + 0j, denormals, real input with signed zeros) and a spectrogram against the oracle (|D| to the last bit: an exactly rounded
    sum / the device's hypot here, NumPy's hypot there); device tensors and NumPy arrays give the same bits."""
    import torch

    y = golden_cases.make_signal("mix", 22050, 61, None, "float32")
    D = L.stft(y)
    S, P = L.magphase(D)
    assert S.dtype == y.dtype and P.dtype == D.dtype and np.allclose(np.abs(P), 1.0) and np.allclose(S * P, D)          # test_magphase
    eS, eP = O.magphase(D)
    assert np.abs(S - eS).max() <= 2.5e-7 * np.abs(eS).max() and np.abs(P - eP).max() <= 3e-7   # (measured: 1.19e-7 = one float32 ulp of the largest |D|, 1.8e-7)
    St, Pt = L.magphase(torch.from_numpy(D).cuda())
    assert isinstance(St, torch.Tensor) and St.is_cuda and np.array_equal(St.cpu().numpy(), S) and np.array_equal(Pt.cpu().numpy(), P)
    Z = np.zeros((128, 128), dtype=np.complex64)                                                                    # test_magphase_zero
    S, P = L.magphase(Z)
    assert S.dtype == np.float32 and P.dtype == np.complex64 and np.all(S == 0) and np.all(P == 1 + 0j)
    Dn = 1.0e-42j * np.ones((128, 128), dtype=np.complex64)                                                         # test_magphase_denormalized
    S, P = L.magphase(Dn)
    assert S.dtype == np.float32 and P.dtype == np.complex64 and np.allclose(S, 1.0e-42) and np.allclose(P, 0 + 1j)
    R = np.array([[-1.0, -0.0], [0.0, 1.0]], dtype=np.float64)                                                      # test_magphase_real
    S, P = L.magphase(R)
    assert S.dtype == np.float64 and P.dtype == np.complex128 and np.array_equal(S, [[1.0, 0.0], [0.0, 1.0]])
    assert np.allclose([[P[0, 0], P[0, 1] ** 2], [P[1, 0], P[1, 1]]], [[-1 + 0j, 1 + 0j], [1 + 0j, 1 + 0j]])
    D64 = D.astype(np.complex128)
    for power in (2, 0.5, 3.5):
        got, exp = L.magphase(D64, power=power), O.magphase(D64, power=power)
        assert got[0].dtype == np.float64 and np.allclose(got[0], exp[0], rtol=1e-13, atol=0) and np.abs(got[1] - exp[1]).max() <= 1e-15


def test_resample_properties(L):
    """Size-independent properties on a batch the oracle would not finish quickly: 64 clips x 30 s at 22 050 Hz -> 16 000 Hz -> back, all
    three converter families; a band-limited signal survives the round trip, lengths are ceil(n * ratio), linearity, and the time axis
    may be any axis."""
    import torch

    sr, n = 22050, 22050 * 30
    t = torch.arange(n, device="cuda", dtype=torch.float64) / sr
    f = torch.linspace(110.0, 3520.0, 64, device="cuda", dtype=torch.float64)[:, None]
    y = (torch.sin(2 * np.pi * f * t) * torch.hann_window(n, device="cuda", dtype=torch.float64)).to(torch.float32)   # tones below 0.45 of the lower Nyquist, faded ends
    for res_type, tol in (("fft", 1e-4), ("polyphase", 2e-2), ("soxr_hq", 1e-4)):
        lo = L.resample(y, orig_sr=sr, target_sr=16000, res_type=res_type)
        assert lo.shape == (64, int(np.ceil(n * 16000 / sr))) and bool(torch.isfinite(lo).all())
        back = L.resample(lo, orig_sr=16000, target_sr=sr, res_type=res_type)
        assert back.shape == y.shape
        err = (back - y)[:, 2000:-2000].abs().max().item()
        assert err <= tol, (res_type, err)
        two = L.resample(2.0 * y[:4] + y[4:8], orig_sr=sr, target_sr=16000, res_type=res_type)
        assert (two - (2.0 * lo[:4] + lo[4:8])).abs().max().item() <= 1e-5
        assert torch.equal(L.resample(y[:3].T.contiguous(), orig_sr=sr, target_sr=16000, res_type=res_type, axis=0).T, lo[:3])


def test_cqt_side_stream_overlap(L):
    """The octave transforms on the context's side stream beside the chain of halvings (lra_ctx_side) against everything on one stream:
    bit-identical, over back-to-back calls without a synchronisation in between (buffers of one call are reused by the next: any ordering
    hole shows up as a difference or a fault), device tensors and NumPy input, fused and two-launch octaves."""
    import torch
    from librosa_amd.core import constantq

    y = torch.from_numpy(golden_cases.make_signal("mix", 22050 * 8, 31, (24,), "float32")).cuda()
    try:
        for fused in (True, False):
            constantq.FUSED_OCTAVES = fused
            constantq.OVERLAP_OCTAVES = False
            ref = L.cqt(y, sr=22050)
            constantq.OVERLAP_OCTAVES = True
            for _ in range(6):
                outs = [L.cqt(y, sr=22050) for _ in range(4)]
                torch.cuda.synchronize()
                assert all(torch.equal(o, ref) for o in outs), fused
            yn = y[:3].cpu().numpy()
            assert np.array_equal(L.cqt(yn, sr=22050), ref[:3].cpu().numpy())
    finally:
        constantq.FUSED_OCTAVES = constantq.OVERLAP_OCTAVES = True


@pytest.mark.parametrize("overlap", [True, False])
def test_cqt_native_recursion_equals_python_loop(L, monkeypatch, overlap):
    """Round 5: the octave recursion as ONE native call (lra_cqt_recursion_exec) against the per-octave calls from Python: bit-identical for cqt and vqt,
    odd lengths (ceil halving), partial lowest octave, stereo, float64, NumPy and device input, with and without the side stream; check_finite=False
    skips only the flag read."""
    import torch
    from librosa_amd.core import constantq

    monkeypatch.setattr(constantq, "OVERLAP_OCTAVES", overlap)
    cases = [dict(y=golden_cases.make_signal("mix", 40001, 3, (2,), "float32"), kw=dict(sr=22050, res_type="polyphase")),
             dict(y=golden_cases.make_signal("chirp", 30000, 4, (), "float32"), kw=dict(sr=22050, n_bins=40, bins_per_octave=12, hop_length=256, res_type="kaiser_fast")),
             dict(y=golden_cases.make_signal("mix", 25000, 5, (3,), "float64"), kw=dict(sr=16000, n_bins=60, fmin=55.0, res_type="polyphase"))]
    for c in cases:
        for dev in (False, True):
            y = torch.from_numpy(c["y"]).cuda() if dev else c["y"]
            monkeypatch.setattr(constantq, "NATIVE_RECURSION", False)
            a = L.cqt(y, **c["kw"])
            av = L.vqt(y, gamma=5.0, **c["kw"])
            monkeypatch.setattr(constantq, "NATIVE_RECURSION", True)
            b = L.cqt(y, **c["kw"])
            bv = L.vqt(y, gamma=5.0, **c["kw"])
            if dev:
                assert torch.equal(a, b) and torch.equal(av, bv)
                assert torch.equal(L.cqt(y, check_finite=False, **c["kw"]), b)
            else:
                assert np.array_equal(a, b) and np.array_equal(av, bv)
    # the three launch orders of the native recursion (ctx option cqt_merge: 1 = octaves 1-2 early on the side stream, round 6; 2 = all behind the chain; 0 = per octave)
    if overlap:
        ctx = L.get_context(0)
        yd = torch.from_numpy(cases[0]["y"]).cuda()
        try:
            outs = []
            for merge in (1, 2, 0, 1):
                ctx.set_option("cqt_merge", merge)
                outs.append(L.cqt(yd, **cases[0]["kw"]))
            assert all(torch.equal(o, outs[0]) for o in outs)
        finally:
            ctx.set_option("cqt_merge", 1)
    bad = torch.from_numpy(cases[0]["y"]).cuda()
    bad[1, 777] = float("nan")
    with pytest.raises(L.ParameterError):
        L.cqt(bad, **cases[0]["kw"])
    L.cqt(bad, check_finite=False, **cases[0]["kw"])  # opt-out does not raise


def test_cqt_many_short_octaves_fork_ring(L, monkeypatch):
    """every octave forks the side stream; each fork now takes its own event out of a ring (16 slots, reused only once the side
    stream is past its wait).  Many short calls with many octaves -- several times round the ring, poisoned outputs, no synchronisation in
    between -- must stay bit-identical to the one-stream order."""
    import torch
    from librosa_amd import _arrays
    from librosa_amd.core import constantq

    y = torch.from_numpy(golden_cases.make_signal("mix", 16384, 5, (3,), "float32")).cuda()
    kw = dict(sr=22050, hop_length=128, n_bins=8 * 12, bins_per_octave=12, fmin=32.7, res_type="polyphase")
    monkeypatch.setattr(constantq, "OVERLAP_OCTAVES", False)
    ref = L.cqt(y, **kw)
    monkeypatch.setattr(constantq, "OVERLAP_OCTAVES", True)
    monkeypatch.setattr(_arrays, "POISON_OUTPUTS", True)
    outs = [L.cqt(y, **kw) for _ in range(40)]   # 8 octaves x 40 calls = 20 times round the ring
    torch.cuda.synchronize()
    assert all(torch.equal(o, ref) for o in outs)


def test_cqt_default_resampler_and_errors(L):
    """The default res_type (soxr_hq in the reference; here the library's own decimator with soxr-HQ's band edges) against the oracle's
    polyphase transform: the two differ by the resamplers' pass-band responses only (2.6e-3 of the peak measured on
    the host; bound 1e-2).  A pure tone lands in its bin; argument errors as in the reference."""
    import cqt_oracle as CQ

    y = golden_cases.make_signal("mix", 44100, 3, None, "float32")
    C = L.cqt(y, sr=22050)
    ref = CQ.cqt(y, sr=22050, res_type="polyphase")
    assert C.shape == ref.shape and C.dtype == np.complex64 and np.abs(C - ref).max() <= 1e-2 * np.abs(ref).max()
    assert np.array_equal(L.cqt(y, sr=22050, res_type="kaiser_best"), C)
    sr = 22050
    for midi in (36, 60, 81):
        f = 440.0 * 2.0 ** ((midi - 69) / 12)
        tone = np.sin(2 * np.pi * f * np.arange(sr) / sr).astype(np.float32)
        mag = np.abs(L.cqt(tone, sr=sr))
        assert mag.shape == (84, 1 + sr // 512) and np.all(np.argmax(mag[:, 5:-5], axis=0) == midi - 24)
    for bad in (dict(tuning=None), dict(fmin=20000.0), dict(n_bins=200), dict(pad_mode="wrap"), dict(hop_length=0), dict(res_type="zero_order_hold"), dict(res_type="linear")):
        with pytest.raises(L.ParameterError):
            L.cqt(y, **bad)
    with pytest.raises(L.ParameterError):
        L.cqt(np.full(4000, np.nan, dtype=np.float32))
    import torch

    with pytest.raises(L.ParameterError):
        L.cqt(torch.full((30000,), float("nan"), device="cuda"))


def test_cqt_full_size(L):
    """BASELINE configs[4]'s batch through the real constant-Q recursion: 64 clips x 30 s, 84 bins, device-resident; sampled clips
    against the oracle, batch == per-clip, timing printed."""
    import cqt_oracle as CQ
    import torch

    Y = torch.from_numpy(O.config_input(64)).cuda()
    C = L.cqt(Y, sr=22050, res_type="polyphase")
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    C = L.cqt(Y, sr=22050, res_type="polyphase")
    ev1.record()
    torch.cuda.synchronize()
    ms_poly = ev0.elapsed_time(ev1)
    Cd = L.cqt(Y, sr=22050)
    torch.cuda.synchronize()
    ev0.record()
    Cd = L.cqt(Y, sr=22050)
    ev1.record()
    torch.cuda.synchronize()
    print(f"cqt 64 x 30 s, 84 bins: polyphase {ms_poly:.2f} ms, default decimator {ev0.elapsed_time(ev1):.2f} ms")
    assert C.shape == (64, 84, 1292) and C.dtype == torch.complex64
    for clip in (0, 41):
        ref = CQ.cqt(Y[clip].cpu().numpy(), sr=22050, res_type="polyphase")
        assert _cqt_close(C[clip].cpu().numpy(), ref)
        assert torch.equal(L.cqt(Y[clip], sr=22050, res_type="polyphase"), C[clip])
        assert (Cd[clip] - C[clip]).abs().max().item() <= 1e-2 * np.abs(ref).max()


# ---- harmonic / percussive separation (librosa/decompose.py:371-528, librosa/effects.py:70-301) ------------------
# The medians are selections (no arithmetic), the masks a handful of float operations: real-valued input reproduces the reference to the
# last bits; complex input goes through |D| first, where NumPy's float32 hypot and the device's differ in the last bit, so everything
# after it is compared at 1e-5 of the peak (float32) / 1e-12 (float64).
def _hpss_close(got, ref, tol):
    return got.shape == ref.shape and got.dtype == ref.dtype and np.abs(got.astype(np.complex128) - ref).max() <= tol * max(np.abs(ref).max(), 1e-30)


def _hpss_golden_body(L):
    import torch

    g = np.load(os.path.join(GOLDEN_DIR, "hpss.npz"))
    D, y = g["D"], g["y"]
    for name, kw in golden_cases.HPSS_CASES.items():
        inp = np.abs(D) ** 2 if name.startswith("power_") else D
        got = L.decompose.hpss(inp, **kw)
        dev = L.decompose.hpss(torch.from_numpy(inp).cuda(), **kw)
        for part, key, d in zip(got, (f"{name}__h", f"{name}__p"), dev):
            ref = g[key]
            assert isinstance(d, torch.Tensor) and d.is_cuda and np.array_equal(d.cpu().numpy(), part), key
            if ref.dtype == bool:   # hard masks: a comparison of two medians; |D|'s last bit may flip a tie
                assert part.dtype == bool and part.shape == ref.shape and np.mean(part != ref) <= 1e-3, key
            elif np.isinf(kw.get("power", 2.0)):   # masked spectra under hard masks: all but a flipped tie within the usual bound
                assert part.shape == ref.shape and part.dtype == ref.dtype and np.mean(np.abs(part - ref) > 1e-5 * np.abs(ref).max()) <= 1e-3, key
            else:
                assert _hpss_close(part, ref, 1e-5), (key, np.abs(part - ref).max() / np.abs(ref).max())
    D64 = D.astype(np.complex128)
    for part, ref in zip(L.decompose.hpss(D64, margin=(1.0, 2.0)), O.hpss(D64, margin=(1.0, 2.0))):
        assert _hpss_close(part, ref, 1e-12)
    # the effects chains: stft -> hpss -> istft, device-resident
    scale = np.abs(y).max()
    h, p = L.effects.hpss(y, n_fft=512, margin=(1.0, 2.0))
    assert h.shape == y.shape and h.dtype == y.dtype and np.abs(h - g["effects_h"]).max() <= 1e-4 * scale and np.abs(p - g["effects_p"]).max() <= 1e-4 * scale
    assert np.abs(L.effects.harmonic(y[0]) - g["effects_harmonic_default"]).max() <= 1e-4 * scale
    assert np.abs(L.effects.percussive(y[0], kernel_size=9, n_fft=1024, hop_length=256) - g["effects_percussive_k9"]).max() <= 1e-4 * scale
    # `window` is accepted and ignored by all three transforms, as in the reference (effects.py:161-183)
    hw, pw_ = L.effects.hpss(y, n_fft=512, margin=(1.0, 2.0), window="hamming")
    assert np.array_equal(hw, h) and np.array_equal(pw_, p)
    ht, pt = L.effects.hpss(torch.from_numpy(y).cuda(), n_fft=512, margin=(1.0, 2.0))
    assert isinstance(ht, torch.Tensor) and ht.is_cuda and np.array_equal(ht.cpu().numpy(), h) and np.array_equal(pt.cpu().numpy(), p)
    for bad in (dict(margin=0.5), dict(margin=(1.0, 0.9)), dict(power=0), dict(kernel_size=0)):
        with pytest.raises(L.ParameterError):
            L.decompose.hpss(D, **bad)


def _hpss_properties_body(L):
    """The reference's own assertions (tests/test_decompose.py: H + P == D, real input, margins; tests/test_effects.py: test_hpss) and
    the BASELINE clip shape: 32 clips x 30 s (32 x 1025 x 1292 complex64) separated on the device, a sampled clip against the oracle."""
    import torch

    rng = np.random.default_rng(33)
    D = (rng.standard_normal((33, 50)) + 1j * rng.standard_normal((33, 50))).astype(np.complex64)
    H_, P_ = L.decompose.hpss(D)
    assert np.allclose(H_ + P_, D, atol=1e-6)
    S = np.abs(D)
    Hs, Ps = L.decompose.hpss(S)
    assert np.allclose(Hs + Ps, S, atol=1e-6) and np.all(Hs >= 0) and np.all(Ps >= 0)
    mh, mp = L.decompose.hpss(S, mask=True)
    assert np.allclose(mh + mp, 1.0, atol=1e-6)
    Hm, Pm = L.decompose.hpss(S, margin=(1.0, 4.0))
    assert np.all(Hm + Pm <= S * (1 + 1e-6))
    Y = torch.from_numpy(O.config_input(32)).cuda()
    Dd = L.stft(Y)
    Hd, Pd = L.decompose.hpss(Dd)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    Hd, Pd = L.decompose.hpss(Dd)
    ev1.record()
    torch.cuda.synchronize()
    print(f"decompose.hpss 32 x 1025 x 1292 complex64: {ev0.elapsed_time(ev1):.2f} ms")
    assert Hd.shape == Dd.shape and Hd.dtype == torch.complex64
    assert (Hd + Pd - Dd).abs().max().item() <= 1e-5 * Dd.abs().max().item()
    clip = 17
    rh, rp = O.hpss(Dd[clip].cpu().numpy())
    assert _hpss_close(Hd[clip].cpu().numpy(), rh, 1e-5) and _hpss_close(Pd[clip].cpu().numpy(), rp, 1e-5)
    h1, p1 = L.decompose.hpss(Dd[clip])
    assert torch.equal(h1, Hd[clip]) and torch.equal(p1, Pd[clip])
    yh, yp = L.effects.hpss(Y[:4])
    eh, ep = O.effects_hpss(Y[1].cpu().numpy())
    scale = float(np.abs(eh).max() + np.abs(ep).max())
    assert np.abs(yh[1].cpu().numpy() - eh).max() <= 1e-4 * scale and np.abs(yp[1].cpu().numpy() - ep).max() <= 1e-4 * scale


def _run_isolated(body):
    """Runs a test body in its own interpreter: the kernels behind it have not been on hardware yet (written after the round's GPU
    minutes were spent), and a device fault there must not take the rest of this suite's report down with it."""
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = (f"import sys; sys.path[:0] = [{here!r}, {os.path.join(root, 'oracle')!r}, {root!r}]; "
            f"import test_gpu_parity as T, librosa_amd as L; T.{body}(L); print('isolated body ok')")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, cwd=root)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "isolated body ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]


def test_hpss_golden():
    _run_isolated("_hpss_golden_body")


def test_hpss_reference_properties_and_full_size():
    _run_isolated("_hpss_properties_body")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hpss_tile_kernel_windows_device(L, dtype):
    """hpss_tile_kernel on the device, the simulator's corner list (tests/test_hostsim.py::test_hpss_tile_kernel_windows): shortest and
    longest windows of both network sizes (run-time window and the compile-time 31), even windows, axes of exactly win + 4, ragged
    tiles, heavy ties, plus windows the element kernel keeps -- real input, so BIT FOR BIT against the oracle; and the element kernel
    (context option hpss_tile = 0) gives the same bits."""
    rng = np.random.default_rng(78)
    cases = [(35, 35, 31, 31), (10, 11, 6, 7), (12, 37, 8, 33), (37, 10, 33, 6), (41, 23, 6, 18), (69, 12, 65, 7), (13, 70, 7, 65), (50, 45, 32, 33), (39, 38, 17, 31), (7, 9, 3, 3),
             (30, 30, 5, 9), (300, 257, 31, 31), (131, 1025, 31, 17)]
    ctx = L.get_context(0)
    for n_frames, n_bins, wh, wp in cases:
        for ties in (False, True):
            S = rng.random((2, n_bins, n_frames)).astype(dtype)
            if ties:
                S = np.round(S * 6).astype(dtype) / 4
            exp = O.hpss(S, kernel_size=(wh, wp), mask=True, power=1.0)
            got = L.decompose.hpss(S, kernel_size=(wh, wp), mask=True, power=1.0)
            assert all(np.array_equal(g, e) and g.dtype == e.dtype for g, e in zip(got, exp)), (n_frames, n_bins, wh, wp, ties)
            try:
                ctx.set_option("hpss_tile", 0)
                assert all(np.array_equal(g, e) for g, e in zip(L.decompose.hpss(S, kernel_size=(wh, wp), mask=True, power=1.0), exp)), (n_frames, n_bins, wh, wp, ties, "element kernel")
            finally:
                ctx.set_option("hpss_tile", 1)


# ---- seeded sweep of the SURVEY 8(f) rows against the oracle (shapes, axes, parameters drawn at random) -------------------------------
@pytest.mark.parametrize("seed", _sweep_seeds())
def test_random_rows_sweep(L, seed):
    """dB conversions, MFCC, PCEN, phase vocoder, harmonic / percussive separation and the constant-Q transform on randomly drawn shapes
    and parameters, NumPy arrays and device tensors, each against the oracle's restatement of the reference with the row's own
    tolerance (the goldens pin the oracle; this pins the device paths away from the golden shapes)."""
    import torch

    import cqt_oracle as CQ

    rng = np.random.default_rng(1000 + seed)
    bad = []

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(6):
            lead = tuple(int(v) for v in rng.integers(1, 4, size=int(rng.integers(0, 3))))
            bands, frames = int(rng.integers(8, 140)), int(rng.integers(5, 300))
            f64 = bool(rng.random() < 0.3)
            S = (rng.standard_normal(lead + (bands, frames)) ** 2 * float(10.0 ** rng.uniform(-6, 3))).astype(np.float64 if f64 else np.float32)
            tol = 1e-10 if f64 else DB_TOL
            # decibel conversions
            kw = dict(ref=[1.0, np.max, np.median, float(rng.uniform(0.1, 5))][int(rng.integers(0, 4))], top_db=[80.0, None, float(rng.uniform(5, 60))][int(rng.integers(0, 3))],
                      amin=float(10.0 ** rng.uniform(-12, -4)))
            for fn in ("power_to_db", "amplitude_to_db"):
                want = getattr(O, fn)(S, **kw)
                # float32: both logarithm terms carry a few ulps of THEIR magnitude (device log10f vs NumPy's), and 10 log10 of a squared
                # amplitude reaches -200 dB while the difference of the two terms stays small: the bar scales with the larger term
                mag = np.square(np.abs(S).astype(np.float64)) if fn == "amplitude_to_db" else np.abs(S).astype(np.float64)
                terms = float(np.abs(10.0 * np.log10(np.maximum(kw["amin"] ** (2 if fn == "amplitude_to_db" else 1), mag))).max())
                tol_fn = tol if f64 else max(tol, 6e-7 * terms)
                for got in (getattr(L, fn)(S, **kw), getattr(L, fn)(dev(S), **kw).cpu().numpy()):
                    if got.shape != want.shape or got.dtype != want.dtype or not np.abs(got - want).max() <= tol_fn:
                        bad.append((fn, S.shape, S.dtype.name, str(kw), float(np.abs(got - want).max())))
            # MFCC from a dB spectrogram
            if bands >= 13:
                mk = dict(n_mfcc=int(rng.integers(2, min(bands, 40))), dct_type=int(rng.integers(1, 4)), norm=[None, "ortho"][int(rng.integers(0, 2))], lifter=[0, 22][int(rng.integers(0, 2))])
                if not (mk["dct_type"] == 1 and mk["norm"] == "ortho" and bands < 2):
                    Sdb = O.power_to_db(S)
                    want = O.mfcc(S=Sdb, **mk)
                    # (float32 sums of up to 140 dB values, times the lifter: unnormalised transforms reach 1e4, so the bar scales with the largest coefficient)
                    ok = lambda a: a.shape == want.shape and (_mfcc_close(a, want) or np.abs(a - want).max() <= (1e-12 if f64 else 2e-6) * np.abs(want).max())
                    got = L.feature.mfcc(S=Sdb, **mk)
                    if not ok(got) or (not f64 and not ok(L.feature.mfcc(S=dev(Sdb), **mk).cpu().numpy())):
                        bad.append(("mfcc", S.shape, S.dtype.name, str(mk), float(np.abs(got - want).max() / np.abs(want).max())))
            # PCEN (general / power == 0 / max-filtered reference, block-wise state)
            pk = dict(gain=float(rng.uniform(0.5, 1.0)), bias=float(rng.choice([2.0, 1.0, 0.5])), power=float(rng.choice([0.5, 0.0, 0.25, 1.0])), time_constant=float(rng.uniform(0.05, 0.6)),
                      eps=float(10.0 ** rng.uniform(-8, -4)), max_size=int(rng.choice([1, 1, 3])), hop_length=int(rng.choice([256, 512])))
            if pk["max_size"] > 1 and S.ndim != 2:
                pk["max_axis"] = -2  # (the reference asks for the band axis explicitly beyond two dimensions, core/spectrum.py:2624-2632)
            want = O.pcen(S, **pk)
            for got in (L.pcen(S, **pk), L.pcen(dev(S), **pk).cpu().numpy()):
                if not _pcen_close(got, want):
                    bad.append(("pcen", S.shape, S.dtype.name, str(pk), float(np.max(np.abs(got - want) / np.abs(want).clip(1e-300)))))
            # phase vocoder and separation on a random complex spectrogram
            bins = int(rng.choice([33, 65, 129, 257]))
            T = int(rng.integers(12, 160))
            D = (rng.standard_normal(lead[:1] + (bins, T)) + 1j * rng.standard_normal(lead[:1] + (bins, T))).astype(np.complex128 if f64 else np.complex64)
            rate = float(rng.choice([0.5, 0.8, 1.0, 1.3, 2.0]))
            want = O.phase_vocoder(D, rate=rate)
            for got in (L.phase_vocoder(D, rate=rate), L.phase_vocoder(dev(D), rate=rate).cpu().numpy()):
                if not _pv_close(got, want):
                    bad.append(("phase_vocoder", D.shape, D.dtype.name, rate))
            hk = dict(kernel_size=[31, (int(rng.integers(3, 40)), int(rng.integers(3, 40))), int(rng.integers(2, 24))][int(rng.integers(0, 3))], power=float(rng.choice([2.0, 1.0, 0.5, np.inf])),
                      margin=[1.0, (1.0, float(rng.uniform(1.0, 4.0)))][int(rng.integers(0, 2))], mask=bool(rng.random() < 0.3))
            X = np.abs(D) if rng.random() < 0.3 else D
            want = O.hpss(X, **hk)
            for got in (L.decompose.hpss(X, **hk), tuple(t.cpu().numpy() for t in L.decompose.hpss(dev(X), **hk))):
                if not all(_hpss_close(a, b, 1e-12 if f64 else 1e-5) for a, b in zip(got, want)):
                    bad.append(("hpss", X.shape, X.dtype.name, str(hk)))
        # constant-Q / variable-Q transform of a short random signal (polyphase decimator: the pinned resampler)
        n = int(rng.integers(9000, 30000))
        y = (rng.standard_normal((2, n)) if rng.random() < 0.5 else rng.standard_normal(n)).astype(np.float32)
        ck = dict(sr=22050, hop_length=int(rng.choice([64, 128, 256, 512])), n_bins=int(rng.choice([24, 36, 48, 60])), bins_per_octave=int(rng.choice([12, 12, 24])), res_type="polyphase",
                  scale=bool(rng.random() < 0.8))
        ck["n_bins"] = max(ck["bins_per_octave"], ck["n_bins"] // ck["bins_per_octave"] * ck["bins_per_octave"])
        try:
            want = CQ.cqt(y, **ck)
        except Exception:  # noqa: BLE001 -- the reference rejects this combination (e.g. the hop does not divide the octave count)
            want = None
        if want is not None:
            for got in (L.cqt(y, **ck), L.cqt(dev(y), **ck).cpu().numpy()):
                if not _cqt_close(got, want):
                    bad.append(("cqt", y.shape, str(ck), float(np.abs(got - want).max() / np.abs(want).max())))
    assert not bad, bad[:6]

