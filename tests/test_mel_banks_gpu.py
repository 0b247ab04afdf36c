"""The fused STFT -> mel launch and the S= product on the MI355X over the bank table of tests/mel_bank_cases.py: every kernel form a bank can take
(context options), per band.

Bar (float32): every element of every non-empty band |M - ref| <= 1e-4 |ref|, no absolute term, against the float64 reference of the same samples and the
same basis values on white noise; rows of empty filters exactly 0; nothing NaN.  float64: 1e-11 |ref| per element.
(tests/test_mel_banks_host.py holds the same banks to the same bar in the simulator, and turns every gate into an assertion.)

Largest |M - ref| / |ref| observed on the MI355X, per form, over all cases, both lengths and powers 2, 1 and 1.5:
  defaults 2.6e-5 (1764 / 44100 / 229 bands),   mixed = 0 (rocFFT path) 2.1e-5,   mixed_pow2_mel = 0 5.3e-6,
  mel_runs = 0 and generic_mel = 1 2.2e-5 (512 / 22050 / 100 bands),   mel_pc = 0, 1, 2 (n_fft 2048) 8.0e-6 (48000 / 256 bands HTK),
  centre = False / reflect padding 1.2e-6,   S= (every layout) 2.2e-6,   float64 4.5e-14 (mixed radix), 1.7e-14 elsewhere;   onset envelope 4.5e-7 of its maximum.
The largest ratios all sit in one-bin bands of frames where that bin happens to be quiet: the band is one |X[k]| ** power, whose error is the FFT's rounding
floor (about 1e-7 of the frame's largest bin in float32) over |X[k]|, and white noise puts a bin 20 to 50 dB under the largest now and then.  Bands that
sum several bins are far quieter cases (simulator, same banks: two-bin bands <= 2.2e-6, three and more bins <= 1.2e-6).
"""
import warnings

import numpy as np
import pytest

import mel_bank_cases as C

pytestmark = pytest.mark.gpu

_EMPTY_MSG = ("Empty filters detected in mel frequency basis. Some channels will produce empty responses. "
              "Try increasing your sampling rate (and fmax) or reducing n_mels.")
_DEFAULTS = dict(mel_pc=1, mel_runs=1, generic_mel=0, mixed=1, mixed_pow2_mel=1)


@pytest.fixture(scope="module")
def L():
    import librosa_amd

    assert librosa_amd.device_count() > 0, "no HIP device: the product has no CPU fallback"
    return librosa_amd


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


_cache = {}


def _inputs(case, n, powers, dtype=np.float32, **stft_kw):
    """(signal, {power: float64 reference}), computed once per (case, length, framing) and left unchanged."""
    key = (C.case_id(case), n, np.dtype(dtype).str, tuple(sorted(stft_kw.items())))
    if key not in _cache:
        y = C.signal(case, n, dtype)
        y.setflags(write=False)
        _cache[key] = (y, {})
    y, refs = _cache[key]
    for p in powers:
        if p not in refs:
            refs[p] = C.reference(case, y, p, **stft_kw)
            refs[p].setflags(write=False)
    return y, refs


def _option_sets(case):
    """The context options that can change which kernel serves this case; every one must meet the reference on its own."""
    n_fft = case[0]
    sets = [("defaults", {})]
    if C.is_pow2(n_fft):
        sets += [("mel_runs=0", dict(mel_runs=0)), ("generic_mel=1", dict(generic_mel=1))]
        if n_fft == 2048:
            sets += [("mel_pc=0", dict(mel_pc=0)), ("mel_pc=1", dict(mel_pc=1)), ("mel_pc=2", dict(mel_pc=2))]
        if n_fft in (128, 256):
            sets += [("mixed_pow2_mel=0", dict(mixed_pow2_mel=0))]
    if n_fft in C.MIXED_SIZES:
        sets += [("mixed=0", dict(mixed=0))]
    return sets


class _options:
    def __init__(self, ctx, opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.ctx.set_option(k, _DEFAULTS[k])


def _mel(L, case, y, power, **extra):
    n_fft, hop, sr, n_mels, kw = case
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the empty-filter warning has its own test)
        return L.feature.melspectrogram(y=y, sr=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels, power=power, **kw, **extra)


_FUSED = [(c, p) for c in C.CASES for p in (2.0, 1.0)] + [(c, 1.5) for c in C.CASES if c[:4] in ((2048, 256, 22050, 128), (2048, 512, 44100, 128)) and not c[4]]


@pytest.mark.parametrize("case,power", _FUSED, ids=[f"{C.case_id(c)}-p{p}" for c, p in _FUSED])
def test_fused_every_form(L, torch, case, power):
    """melspectrogram(y=...) under each option set: NumPy input == device tensor bit for bit, each against the float64 reference at the per-element bar,
    no NaN, empty filters exactly 0; clip i of the batch == clip i alone."""
    ctx = L.get_context(0)
    B = C.basis(case)
    worst = {}
    for li, n in enumerate(C.signal_lengths(case)):
        y, refs = _inputs(case, n, (power,))
        ref = refs[power]
        yt = torch.from_numpy(np.array(y)).to("cuda:0")
        for name, opts in _option_sets(case):
            with _options(ctx, opts):
                Md = _mel(L, case, yt, power)
                assert torch.is_tensor(Md) and Md.device.type == "cuda"
                Md = Md.cpu().numpy()
                Mh = _mel(L, case, np.array(y), power) if li == 0 else None
                alone = [_mel(L, case, yt[i], power).cpu().numpy() for i in range(C.BATCH)] if (li == 1 or name == "defaults") else None
            assert Md.dtype == np.float32
            r = C.worst_ratio(Md, ref, B)
            worst[name] = max(worst.get(name, 0.0), r)
            if Mh is not None:
                assert isinstance(Mh, np.ndarray) and np.array_equal(Mh, Md), name
            if alone is not None:
                for i in range(C.BATCH):
                    assert np.array_equal(alone[i], Md[i]), (name, i)
    print(f"mel banks {C.case_id(case)} power {power}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= C.F32_BAR}
    assert not bad, bad


def _identity_blocks(n_bins, dtype, width=2048):
    for k0 in range(0, n_bins, width):
        k1 = min(n_bins, k0 + width)
        S = np.zeros((n_bins, k1 - k0), dtype=dtype)
        S[np.arange(k0, k1), np.arange(k1 - k0)] = 1
        yield k0, k1, S


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_apply_identity_returns_the_basis(L, torch, case):
    """S = eye(n_bins) through lra_mel_apply_exec returns filters.mel's basis exactly: every stored weight and every band's c0 / len / off
    (in column blocks where n_bins is large; as a host array, C-ordered, and as the frame-major device view)."""
    n_fft, hop, sr, n_mels, kw = case
    f64_too = case[:4] in ((2048, 512, 48000, 256), (512, 128, 44100, 128))
    for dtype in (np.float32, np.float64) if f64_too else (np.float32,):
        B = C.basis(case, dtype)
        for k0, k1, S in _identity_blocks(B.shape[1], dtype):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                M = L.feature.melspectrogram(S=S, sr=sr, n_fft=n_fft, n_mels=n_mels, dtype=dtype, **kw)
                St = torch.from_numpy(np.ascontiguousarray(S.T)).to("cuda:0").transpose(-1, -2)  # (n_bins, T) view of [t][f] memory
                Mt = L.feature.melspectrogram(S=St, sr=sr, n_fft=n_fft, n_mels=n_mels, dtype=dtype, **kw).cpu().numpy()
            assert M.dtype == dtype and M.shape == (n_mels, k1 - k0)
            assert np.array_equal(M, B[:, k0:k1]) and np.array_equal(Mt, B[:, k0:k1])


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_apply_random_spectrum(L, torch, case):
    """A random non-negative S against the float64 product, per element, in the layouts _apply_mel distinguishes: C-ordered (host and device), the
    frame-major view _spectrogram returns for device tensors, and that view with padded rows."""
    n_fft, hop, sr, n_mels, kw = case
    B = C.basis(case)
    n_bins = B.shape[1]
    rng = np.random.default_rng([n_fft, n_mels, 5])
    T = 261  # (two blocks of 256 frames in mel_apply_kernel, the second nearly empty)
    S = rng.random((2, n_bins, T), dtype=np.float32) + np.float32(0.01)
    ref = np.einsum("mf,bft->bmt", B.astype(np.float64), S.astype(np.float64))
    Sd = torch.from_numpy(S).to("cuda:0")
    fm = Sd.transpose(-1, -2).contiguous().transpose(-1, -2)
    wide = torch.zeros((2, T, n_bins + 7), dtype=Sd.dtype, device=Sd.device)
    wide[..., :n_bins] = Sd.transpose(-1, -2)
    layouts = dict(host=S, device=Sd, frame_major=fm, padded_rows=wide[..., :n_bins].transpose(-1, -2))
    worst = {}
    for name, s in layouts.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            M = L.feature.melspectrogram(S=s, sr=sr, n_fft=n_fft, n_mels=n_mels, **kw)
        M = M.cpu().numpy() if torch.is_tensor(M) else M
        worst[name] = C.worst_ratio(M, ref, B)
    print(f"mel banks S= {C.case_id(case)}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= C.F32_BAR, worst


_F64_CASES = [c for c in C.CASES if (c[:4], tuple(sorted(c[4]))) in (((2048, 512, 22050, 128), ()), ((2048, 512, 48000, 256), ("fmax", "fmin", "htk")), ((2048, 512, 22050, 1), ()),
                                                                      ((512, 128, 22050, 101), ()), ((256, 64, 8000, 56), ()), ((400, 160, 16000, 128), ()))]


@pytest.mark.parametrize("case", _F64_CASES, ids=C.case_id)
def test_float64_input(L, torch, case):
    """One bank per gate family in float64 (an empty-filter bank and a one-band bank among them): 1e-11 |ref| per element under each option set."""
    assert len(_F64_CASES) == 6
    ctx = L.get_context(0)
    B = C.basis(case)  # (filters.mel's default dtype: float32 values, applied in float64)
    worst = {}
    for n in C.signal_lengths(case):
        for power in (2.0, 1.0):
            y, refs = _inputs(case, n, (power,), np.float64)
            yt = torch.from_numpy(np.array(y)).to("cuda:0")
            for name, opts in _option_sets(case):
                with _options(ctx, opts):
                    Md = _mel(L, case, yt, power).cpu().numpy()
                    Mh = _mel(L, case, np.array(y), power)
                assert Md.dtype == np.float64 and np.array_equal(Mh, Md)
                worst[name] = max(worst.get(name, 0.0), C.worst_ratio(Md, refs[power], B))
    print(f"mel banks float64 {C.case_id(case)}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= C.F64_BAR, worst


@pytest.mark.parametrize("stft_kw", [dict(center=False), dict(pad_mode="reflect")], ids=["uncentred", "reflect"])
def test_served_bank_other_framing(L, torch, stft_kw):
    """A bank the producer / consumer kernel serves (127 bands, hop 256), uncentred and reflect-padded, with that kernel and without."""
    case = (2048, 256, 22050, 127, {})
    ctx = L.get_context(0)
    B = C.basis(case)
    for n in C.signal_lengths(case, center=stft_kw.get("center", True)):
        for power in (2.0, 1.0):
            y, refs = _inputs(case, n, (power,), **stft_kw)
            yt = torch.from_numpy(np.array(y)).to("cuda:0")
            for pc in (1, 0):
                with _options(ctx, dict(mel_pc=pc)):
                    M = _mel(L, case, yt, power, **stft_kw).cpu().numpy()
                r = C.worst_ratio(M, refs[power], B)
                print(f"mel banks framing {stft_kw} n {n} power {power} mel_pc {pc}: {r:.2e}")
                assert r <= C.F32_BAR


def test_onset_strength_reaches_the_same_plan(L, torch):
    """onset_strength(y=..., n_mels=127, fmax=8000): its mel kwargs reach the plan of a served 127-band bank; against the float64 restatement of
    tests/test_onset_gpu.py built from this package's mel spectrogram, which itself meets the per-element bar."""
    from test_onset_gpu import _restate_f64

    case = (2048, 512, 22050, 127, dict(fmax=8000))
    n = C.signal_lengths(case)[1] + 16 * 512
    y, refs = _inputs(case, n, (2.0,))
    yt = torch.from_numpy(np.array(y)).to("cuda:0")
    M = _mel(L, case, yt, 2.0).cpu().numpy()
    assert C.worst_ratio(M, refs[2.0], C.basis(case)) <= C.F32_BAR
    got = L.onset.onset_strength(y=yt, sr=22050, n_mels=127, fmax=8000).cpu().numpy()
    want = _restate_f64(M)[:, 0, :]
    assert got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()
    print(f"mel banks onset 127 bands fmax 8000: max |err| / max |ref| = {err:.3e}")
    assert err <= 1e-5


@pytest.mark.parametrize("case", [c for c in C.CASES if C.case_id(c) in C.EMPTY_FILTERS] + [(2048, 512, 22050, 128, {})], ids=C.case_id)
def test_empty_filter_warning(L, case):
    """filters.mel warns about empty filters as the reference does (librosa/filters.py:241-249: one UserWarning, this text), on every call of
    melspectrogram too; not for a bank without empty filters, nor for the one whose only empty filter starts at 0 Hz."""
    n_fft, hop, sr, n_mels, kw = case
    y = np.array(_inputs(case, C.signal_lengths(case)[0], ())[0])
    calls = (lambda: L.filters.mel(sr=sr, n_fft=n_fft, n_mels=n_mels, **kw),
             lambda: L.feature.melspectrogram(y=y, sr=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels, **kw),
             lambda: L.feature.melspectrogram(y=y, sr=sr, n_fft=n_fft, hop_length=hop, n_mels=n_mels, **kw))
    for call in calls:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            call()
        if C.case_id(case) in C.EMPTY_FILTER_WARNS:
            assert [(w.category, str(w.message)) for w in caught] == [(UserWarning, _EMPTY_MSG)]
        else:
            assert not caught

