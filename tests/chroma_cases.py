"""The inputs, cases, float64 model and bound of tests/golden/chroma.npz, rebuilt from seeds (scripts/make_chroma_golden.py stores only the
reference's results, the inputs' and filter banks' checksums).

Bound (the project's own, tests/mel_bank_cases.py): against the float64 model -- the float64 einsum of the bank as stored with the float64
spectrogram, the threshold, the float64 ``normalize`` -- ``|got - model| <= BAR * max |model| over the frame's elements`` with BAR = 1e-4 for
float32 and 1e-11 for float64.  Relative to the frame's largest element: a tonal frame's near-empty chroma bins are not held to a relative
error on leakage.  The generator asserts that the reference's own result lies within a tenth of it."""
import hashlib
import os

import numpy as np

F32_BAR, F64_BAR = 1e-4, 1e-11  # the bars of tests/mel_bank_cases.py (tests/test_chroma_host.py asserts that they are the same)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chroma.npz")
SR = 22050

# csrc/lra_chroma.h (tests/test_chroma_host.py checks them against the header): frames a wave carries at once, frames a workgroup takes per
# pass, frames per workgroup of the frame-major kernel, frames per workgroup of the bin-major kernel, rows per chunk
FR, PASS, TILE_F, COLS_F, ROWS = 4, 16, 64, 256, 12

INF = float("inf")


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- filter banks: name -> kwargs -----------------------------------------------------------------------------------------------------
BANKS = {f"n{n}": dict(sr=SR, n_fft=n) for n in (64, 400, 512, 1000, 2048, 4096)}
for _c in (5, 12, 24, 36, 50):
    BANKS[f"c{_c}"] = dict(sr=SR, n_fft=512, n_chroma=_c)
BANKS.update(
    tune_up=dict(sr=SR, n_fft=2048, tuning=0.3), tune_down=dict(sr=SR, n_fft=2048, tuning=-0.3), tune_c36=dict(sr=SR, n_fft=512, n_chroma=36, tuning=0.3),
    flat=dict(sr=SR, n_fft=512, octwidth=None), base_a=dict(sr=SR, n_fft=512, base_c=False), base_a_c24=dict(sr=SR, n_fft=512, base_c=False, n_chroma=24),
    norm_none=dict(sr=SR, n_fft=512, norm=None), norm_1=dict(sr=SR, n_fft=512, norm=1), norm_inf=dict(sr=SR, n_fft=512, norm=INF),
    f64=dict(sr=SR, n_fft=512, dtype="float64"), sr16k=dict(sr=16000, n_fft=400, ctroct=4.0, octwidth=1.5), odd=dict(sr=SR, n_fft=501))
_WIN = [0.25, 0.5, 0.25]
CQ_BANKS = {
    "b12_84": (84, dict()), "b36_252": (252, dict(bins_per_octave=36)), "b36_250": (250, dict(bins_per_octave=36)), "b24_c24": (96, dict(bins_per_octave=24, n_chroma=24)),
    "b36_c36": (108, dict(bins_per_octave=36, n_chroma=36)), "b60_c5": (120, dict(bins_per_octave=60, n_chroma=5)), "b100_c50": (200, dict(bins_per_octave=100, n_chroma=50)),
    "base_a": (84, dict(base_c=False)), "fmin_a1": (84, dict(fmin=55.0)), "fmin_odd": (252, dict(bins_per_octave=36, fmin=40.0)), "window": (252, dict(bins_per_octave=36, window=_WIN)),
    "window_b12": (84, dict(window=_WIN)), "f64": (84, dict(dtype="float64")), "c24_b12_err": (84, dict(bins_per_octave=12, n_chroma=24)),
}
BANK_ERRORS = {"neg_norm": dict(sr=SR, n_fft=512, norm=-1), "str_norm": dict(sr=SR, n_fft=512, norm="l2")}


def bank_kwargs(kw):
    kw = dict(kw)
    if "dtype" in kw:
        kw["dtype"] = np.dtype(kw["dtype"])
    if "window" in kw:
        kw["window"] = np.asarray(kw["window"])
    return kw


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def power_spec(seed, lead, n_bins, n_frames, dtype):
    """A non-negative spectrogram with a tilt, a broadband floor and a few strong partials per frame."""
    rng = np.random.default_rng(seed)
    shape = tuple(lead) + (n_bins, n_frames)
    x = rng.standard_normal(shape) ** 2 / (1.0 + np.arange(n_bins)[:, None] / 40.0)
    for _ in range(3):
        f = rng.integers(1, max(2, n_bins), size=tuple(lead) + (1, n_frames))
        np.put_along_axis(x, f, 50.0 * (1.0 + rng.random(f.shape)), axis=-2)
    return x.astype(dtype)


def signal(seed, lead, n):
    """Three partials over a noise floor, float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    y = np.zeros(tuple(lead) + (n,))
    for _ in range(3):
        f = rng.uniform(80.0, 4000.0, size=tuple(lead) + (1,))
        y += rng.uniform(0.2, 1.0, size=f.shape) * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28, size=f.shape))
    return (y + 0.01 * rng.standard_normal(y.shape)).astype(np.float32)


def zero_spec(seed, n_bins, n_frames):
    """Two clips: one with a stretch of zero frames in the middle, one all zero."""
    x = np.zeros((2, n_bins, n_frames), np.float32)
    x[0] = power_spec(seed, (), n_bins, n_frames, np.float32)
    x[0, :, n_frames // 3 : n_frames // 3 + 9] = 0
    return x


# ---- chroma_stft(S=...): name -> dict(seed, n_fft, frames, lead, dtype, kw).  kw: the call's keywords (tuning always a number) --------------
def _s(seed, n_fft, frames, lead=(), dtype="float32", **kw):
    return dict(seed=seed, n_fft=n_fft, frames=frames, lead=lead, dtype=dtype, kw=dict(dict(sr=SR, tuning=0.0), **kw))


STFT_S = {
    # bin counts off the wave width x the frame counts 1, 63, 64, 65, one off the frames-per-wave block (70 = TILE_F + 6, 6 % FR != 0) and
    # one off the workgroup's tile (130 = 2 TILE_F + 2); 300 frames: more than one workgroup of the bin-major kernel (COLS_F = 256)
    "n64_t1": _s(1, 64, 1), "n400_t63": _s(2, 400, 63), "n512_t64": _s(3, 512, 64), "n2048_t65": _s(4, 2048, 65), "n1000_t70": _s(5, 1000, 70),
    "n2048_t130": _s(6, 2048, 130), "n512_t300": _s(7, 512, 300), "n4096_t20": _s(8, 4096, 20),
    "c5": _s(9, 512, 70, n_chroma=5), "c36": _s(10, 512, 70, n_chroma=36, tuning=0.3), "c50": _s(11, 512, 70, n_chroma=50), "c24_n2048": _s(12, 2048, 20, n_chroma=24),
    "norm1": _s(13, 512, 65, norm=1), "norm2": _s(14, 512, 65, norm=2), "norm_none": _s(15, 512, 65, norm=None), "norm1_c50": _s(16, 512, 65, norm=1, n_chroma=50),
    "norm2_c36": _s(17, 400, 65, norm=2, n_chroma=36), "norm_none_c50": _s(18, 512, 65, norm=None, n_chroma=50),
    "norm0": _s(19, 512, 65, norm=0), "norm_neg_inf": _s(20, 512, 65, norm=-INF), "norm3": _s(21, 512, 65, norm=3.0),
    "batch3": _s(22, 400, 70, lead=(3,)), "batch2x2": _s(23, 512, 65, lead=(2, 2), norm=2), "batch3_c50": _s(24, 64, 130, lead=(3,), n_chroma=50),
    "f64": _s(25, 512, 65, dtype="float64"), "f64_c50_norm2": _s(26, 2048, 20, dtype="float64", n_chroma=50, norm=2), "f64_bank": _s(27, 512, 65, dtype_bank="float64"),
    "tuned": _s(28, 2048, 20, tuning=-0.3), "flat": _s(29, 512, 65, octwidth=None, base_c=False),
    "zeros": dict(seed=30, n_fft=512, frames=70, lead=(2,), dtype="float32", kw=dict(sr=SR, tuning=0.0), zero=True),
    "zeros_norm2": dict(seed=31, n_fft=512, frames=70, lead=(2,), dtype="float32", kw=dict(sr=SR, tuning=0.0, norm=2), zero=True),
}


def stft_s_input(case):
    c = STFT_S[case]
    n_bins = 1 + c["n_fft"] // 2
    if c.get("zero"):
        return zero_spec(c["seed"], n_bins, c["frames"])
    return power_spec(c["seed"], c["lead"], n_bins, c["frames"], np.dtype(c["dtype"]))


def call_kwargs(kw):
    """The case's keywords as the functions take them (``dtype_bank`` is filters.chroma's ``dtype``)."""
    kw = dict(kw)
    if "dtype_bank" in kw:
        kw["dtype"] = np.dtype(kw.pop("dtype_bank"))
    if isinstance(kw.get("window"), list):
        kw["window"] = np.asarray(kw["window"])
    return kw


# ---- chroma_stft(y=...): name -> dict(seed, n, lead, kw) ------------------------------------------------------------------------------------
def _y(seed, n_fft, frames, lead=(), **kw):
    hop = max(1, n_fft // 4)
    return dict(seed=seed, n=hop * (frames - 1), lead=lead, kw=dict(dict(sr=SR, tuning=0.0, n_fft=n_fft, hop_length=hop), **kw))


STFT_Y = {
    "y_n64": _y(40, 64, 65), "y_n400": _y(41, 400, 70), "y_n512": _y(42, 512, 63), "y_n1000": _y(43, 1000, 70), "y_n2048": _y(44, 2048, 130, hop_length=512),
    "y_n4096": _y(45, 4096, 20, hop_length=512), "y_batch3": _y(46, 512, 70, lead=(3,), norm=2), "y_c50": _y(47, 400, 65, n_chroma=50, norm=1), "y_norm3": _y(48, 512, 65, norm=3.0),
    "y_win": _y(49, 512, 65, win_length=400, window="hamming", center=False),
}


def stft_y_input(case):
    c = STFT_Y[case]
    return signal(c["seed"], c["lead"], c["n"])


# ---- chroma_cqt(C=...): name -> dict(seed, n_input, frames, lead, dtype, kw) -----------------------------------------------------------------
def _c(seed, n_input, frames, lead=(), dtype="float32", **kw):
    return dict(seed=seed, n_input=n_input, frames=frames, lead=lead, dtype=dtype, kw=kw)


# positive thresholds: each lies in the widest gap of its case's raw values between their 3rd and 20th percentile, so that it decides some
# elements either way and none is close (the generator certifies: no float64 raw value within 1e-3 of the threshold)
CQT_C = {
    "b12_t65": _c(60, 84, 65, bins_per_octave=12), "b36_t70": _c(61, 252, 70), "b36_none": _c(62, 252, 70, threshold=None), "b36_thr": _c(63, 252, 130, threshold=5.866),
    "b36_thr_norm2": _c(64, 252, 65, threshold=5.729, norm=2), "b36_thr_none": _c(65, 252, 65, threshold=5.907, norm=None), "b12_t300": _c(66, 84, 300, bins_per_octave=12, norm=1),
    "c36": _c(67, 108, 65, n_chroma=36, bins_per_octave=36), "c50": _c(68, 200, 70, n_chroma=50, bins_per_octave=100, threshold=0.651), "c5": _c(69, 120, 63, n_chroma=5, bins_per_octave=60),
    "batch3": _c(70, 252, 70, lead=(3,), threshold=6.02), "f64": _c(71, 252, 65, dtype="float64", threshold=5.974), "window": _c(72, 252, 65, window=_WIN),
    "fmin": _c(73, 250, 64, fmin=40.0), "norm0": _c(74, 84, 65, bins_per_octave=12, norm=0), "t1": _c(75, 84, 1, bins_per_octave=12),
}


def cqt_c_input(case):
    c = CQT_C[case]
    rng = np.random.default_rng(c["seed"])
    x = np.abs(rng.standard_normal(tuple(c["lead"]) + (c["n_input"], c["frames"]))) / (1.0 + np.arange(c["n_input"])[:, None] / 100.0)
    return x.astype(np.dtype(c["dtype"]))


# ---- chroma_cqt(y=...): about 2 s; the converter is "polyphase" on both sides (the reference's default needs soxr) ----------------------------
CQT_Y = {"y_2s": dict(seed=80, n=44100, lead=(), kw=dict(sr=SR, tuning=0.0, threshold=0.0)),
         "y_2s_thr": dict(seed=81, n=44100, lead=(), kw=dict(sr=SR, tuning=0.0, threshold=0.565, norm=2))}
CQT_RES_TYPE = "polyphase"


def cqt_y_input(case):
    c = CQT_Y[case]
    return signal(c["seed"], c["lead"], c["n"])


def cqt_dims(kw):
    bpo = kw.get("bins_per_octave", 36)
    return kw.get("n_octaves", 7) * bpo, bpo


# ---- argument errors (no device work): name -> (function, kwargs) ---------------------------------------------------------------------------
ERRORS = {
    "stft_nothing": ("chroma_stft", dict(tuning=0.0)),
    "stft_no_n_fft": ("chroma_stft", dict(tuning=0.0, n_fft=None, y="y")),
    "cqt_nothing": ("chroma_cqt", dict(tuning=0.0)),
    "cqt_bpo": ("chroma_cqt", dict(tuning=0.0, y="y", bins_per_octave=30, n_chroma=12)),
    "cqt_bpo_C": ("chroma_cqt", dict(C="C84", bins_per_octave=30, n_chroma=12)),
    "cqt_bad_norm_C": ("chroma_cqt", dict(C="C84", bins_per_octave=None, n_chroma=24, norm=-1)),
}


# ---- the model and the bound --------------------------------------------------------------------------------------------------------------
def model(bank, x, norm, threshold, out_dtype):
    """float64 einsum of the bank as stored with the float64 spectrogram, the threshold, the float64 normalize (lengths below ``tiny`` of the
    result dtype are left alone).  Returns (normalised model, raw values before the threshold)."""
    raw = np.einsum("cf,...ft->...ct", bank.astype(np.float64), np.asarray(x, dtype=np.float64))
    cut = raw.copy()
    if threshold is not None:
        cut[cut < threshold] = 0.0
    if norm is None:
        return cut, raw
    mag = np.abs(cut)
    if norm == INF:
        length = mag.max(axis=-2, keepdims=True)
    elif norm == -INF:
        length = mag.min(axis=-2, keepdims=True)
    elif norm == 0:
        length = (mag > 0).sum(axis=-2, keepdims=True).astype(np.float64)
    else:
        length = (mag**norm).sum(axis=-2, keepdims=True) ** (1.0 / norm)
    length = np.where(length < np.finfo(np.dtype(out_dtype)).tiny, 1.0, length)
    return cut / length, raw


def worst(got, mod, out_dtype):
    """max over the array of |got - model| / (largest magnitude of the frame) -- to be at most BAR; frames whose model is all zero must be
    exactly zero and count as 0."""
    scale = np.abs(mod).max(axis=-2, keepdims=True)
    err = np.abs(np.asarray(got, dtype=np.float64) - mod)
    dead = np.broadcast_to(scale == 0, err.shape)
    if np.any(err[dead] != 0):
        return INF
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(dead, 0.0, err / scale)
    return float(rel.max()) if rel.size else 0.0


def bar(out_dtype):
    return F64_BAR if np.dtype(out_dtype) == np.float64 else F32_BAR


def result_dtype(x_dtype, bank_dtype):
    return np.dtype(np.float64) if (np.dtype(x_dtype) == np.float64 or np.dtype(bank_dtype) == np.float64) else np.dtype(np.float32)


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------------
def load():
    """(npz, meta): the reference's results and the JSON record of digests, exception names and the generator's own measurements."""
    import json

    z = np.load(GOLDEN)
    return z, json.loads(bytes(z["meta"]).decode())


BANK_KEYS = ("n_chroma", "tuning", "ctroct", "octwidth", "base_c", "dtype")
CQ_BANK_KEYS = ("bins_per_octave", "n_chroma", "fmin", "window")


def stft_bank_kwargs(kw, n_fft):
    """filters.chroma's keywords of a chroma_stft case."""
    return dict({k: v for k, v in kw.items() if k in BANK_KEYS}, sr=kw["sr"], n_fft=n_fft)


def cqt_bank_kwargs(kw):
    """filters.cq_to_chroma's keywords of a chroma_cqt case (chroma_cqt's default is 36 bins per octave, the filter's own is 12)."""
    return dict({"bins_per_octave": 36}, **{k: v for k, v in kw.items() if k in CQ_BANK_KEYS})
