"""Cases, inputs and the NumPy model of ``piptrack`` / ``pitch_tuning`` / ``estimate_tuning`` shared by ``scripts/make_pitch_golden.py``,
``tests/test_pitch_host.py`` and ``tests/test_pitch_gpu.py``.

TEST INFRASTRUCTURE ONLY.  Inputs come from seeds; ``tests/golden/pitch.npz`` holds the unmodified reference's results, digests of the
inputs and exception names.  The model follows ``librosa/core/pitch.py:28-366`` line by line in the dtype it is handed (hand it float64
arrays for the float64 model).

Bounds.  ``piptrack(S=...)`` sees the very bits the reference saw, so every comparison that decides a peak is exact: the non-zero patterns
must be equal.  Values: ``a`` and ``b`` of the parabola are the same whether or not a multiply-add is fused (the factors 2 and 0.5 are
exact), ``-b / a`` is one IEEE division, ``pitches`` one rounding of a float64 expression, and ``S + 0.5 * avg * shift`` may be fused where
NumPy rounds twice: about 1 ulp.  The bound is ``ULPS`` = 4 units in the last place of the result dtype.
"""
from __future__ import annotations

import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pitch.npz")
SR = 22050
ULPS = 4
STAGE_TILE = 1088  # bins the frame-major kernel stages at a time (csrc/lra_pitch.h: kTile); the seam cases sit on it
REFS = {"mean": np.mean, "max": np.max, "median": np.median}


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def resolve_ref(ref):
    return REFS[ref] if isinstance(ref, str) else ref


# ---- piptrack(S=...) cases ------------------------------------------------------------------------------------------------------------------
# name -> dict(seed, lead, n_bins, n_frames, dtype, layout ("fm": frames major, the device layout behind a (..., f, t) view; "bm": C-contiguous
# (..., f, t)), kind ("random", "complex", "negative", "seam", "shapes", "last"), kw (piptrack's keyword arguments))
WIDE = dict(fmin=0.0, fmax=float(SR))  # every bin below sr / 2 (fmax > sr / 2 is clipped)
PIP = {}


def _add(name, **c):
    c.setdefault("lead", ())
    c.setdefault("dtype", "float32")
    c.setdefault("kind", "random")
    c.setdefault("kw", {})
    c["kw"] = dict(sr=SR, **c["kw"]) if "sr" not in c["kw"] else dict(c["kw"])
    c.setdefault("seed", 1000 + len(PIP))
    PIP[name] = c


for _n in (2, 3, 33, 65, 257, 1025, 2049):
    for _layout in ("fm", "bm"):
        _add(f"bins{_n}_{_layout}", n_bins=_n, n_frames=5, layout=_layout, kw=WIDE)
_add("bins1025_default", n_bins=1025, n_frames=9, layout="fm")  # the defaults: 150 .. 4000 Hz
_add("seam_fm", n_bins=2049, n_frames=6, layout="fm", kind="seam", kw=WIDE)
_add("seam_fm64", n_bins=2049, n_frames=6, layout="fm", kind="seam", dtype="float64", kw=WIDE)
for _t in (1, 63, 64, 65):
    for _layout in ("fm", "bm"):
        _add(f"frames{_t}_{_layout}", n_bins=33, n_frames=_t, layout=_layout, kw=WIDE)
_add("frames300_bm", n_bins=9, n_frames=300, layout="bm", kw=WIDE)  # more than one workgroup of the bin-major kernel (256 frames)
for _lead in ((), (2,), (2, 3)):
    for _dt in ("float32", "float64"):
        for _layout in ("fm", "bm"):
            _add(f"lead{len(_lead)}_{_dt}_{_layout}", lead=_lead, n_bins=65, n_frames=7, dtype=_dt, layout=_layout, kw=WIDE)
_add("complex_fm", n_bins=65, n_frames=9, layout="fm", kind="complex", kw=WIDE)
_add("complex_bm", n_bins=65, n_frames=9, layout="bm", kind="complex", lead=(2,), kw=WIDE)
_add("complex128_bm", n_bins=33, n_frames=5, layout="bm", kind="complex", dtype="float64", kw=WIDE)
_add("negative_fm", n_bins=65, n_frames=9, layout="fm", kind="negative", kw=WIDE)
_add("negative_bm", n_bins=65, n_frames=9, layout="bm", kind="negative", kw=WIDE)
# crafted frames: a plateau (only its first bin is a peak), a straight ramp (a == 0: |b| >= |a|, no shift), an all-zero and a constant frame, a
# peak at bin 1, and noise
_add("shapes_fm", n_bins=9, n_frames=6, layout="fm", kind="shapes", kw=WIDE)
_add("shapes_bm", n_bins=9, n_frames=6, layout="bm", kind="shapes", kw=WIDE)
_add("shapes_bm64", n_bins=9, n_frames=6, layout="bm", kind="shapes", dtype="float64", kw=WIDE)
# an odd n_fft: the last bin lies below sr / 2 and passes the mask; there shift is 0 and mags == S
_add("last_fm", n_bins=33, n_frames=8, layout="fm", kind="last", kw=dict(n_fft=65, **WIDE))
_add("last_bm", n_bins=33, n_frames=8, layout="bm", kind="last", kw=dict(n_fft=65, **WIDE))
# sr 6400, n_fft 64: bin f is at 100 f Hz exactly; fmin is inclusive, fmax exclusive
_add("ends_fm", n_bins=33, n_frames=9, layout="fm", kw=dict(sr=6400, fmin=300.0, fmax=1500.0))
_add("ends_bm", n_bins=33, n_frames=9, layout="bm", kw=dict(sr=6400, fmin=300.0, fmax=1500.0))
_add("thr0_fm", n_bins=65, n_frames=9, layout="fm", kw=dict(threshold=0.0, **WIDE))
_add("thr1_bm", n_bins=65, n_frames=9, layout="bm", kw=dict(threshold=1.0, **WIDE))
_add("refnum_fm", n_bins=65, n_frames=9, layout="fm", kw=dict(ref=0.3, **WIDE))
_add("refnum_neg_bm", n_bins=65, n_frames=9, layout="bm", kw=dict(ref=-0.5, **WIDE))
_add("refmean_fm", n_bins=65, n_frames=9, layout="fm", lead=(2,), kw=dict(ref="mean", threshold=1.0, **WIDE))
_add("refmean_bm", n_bins=65, n_frames=9, layout="bm", kw=dict(ref="mean", threshold=1.0, **WIDE))
_add("refmax_bm", n_bins=65, n_frames=9, layout="bm", kw=dict(ref="max", **WIDE))


def pip_input(name):
    """The (..., n_bins, n_frames) input of a case: a view of a (..., n_frames, n_bins) array for layout "fm"."""
    c = PIP[name]
    rng = np.random.default_rng(c["seed"])
    shape = tuple(c["lead"]) + (c["n_frames"], c["n_bins"])
    dtype = np.dtype(c["dtype"])
    x = rng.random(shape) ** (3 if c["n_bins"] < 257 else 24)  # (..., t, f): a few bins per frame stand out (fewer in the long rows: a small fixture)
    kind = c["kind"]
    if kind == "negative":
        x = x * np.where(rng.random(shape) < 0.3, -1.0, 1.0)
    elif kind == "complex":
        x = x * np.exp(2j * np.pi * rng.random(shape))
    elif kind == "seam":
        x = 0.01 + 0.01 * rng.random(shape)
        for t, f in enumerate((STAGE_TILE - 1, STAGE_TILE, STAGE_TILE + 1, STAGE_TILE - 2, 2 * STAGE_TILE - 1 - 128, 1)):
            x[..., t, f] = 1.0 + 0.1 * t
            x[..., t, f + 1] = 0.6
        x[..., 0, STAGE_TILE] = 1.0  # a plateau across the seam: only its first bin, the tile's last, is a peak
    elif kind == "shapes":
        x[..., 0, :] = [0, 1, 3, 3, 1, 0, 0.5, 0.25, 0]
        x[..., 1, :] = np.arange(9) / 8.0
        x[..., 2, :] = 0.0
        x[..., 3, :] = 0.7
        x[..., 4, :] = [0, 2, 1, 0, 0, 0.5, 0.75, 0.5, 0]
    elif kind == "last":
        x[..., ::2, -1] = 1.5  # every other frame peaks at the last bin
    x = x.astype(np.complex64 if dtype == np.float32 else np.complex128) if kind == "complex" else x.astype(dtype)
    x = np.ascontiguousarray(x)
    view = np.swapaxes(x, -1, -2)
    return view if c["layout"] == "fm" else np.ascontiguousarray(view)


def pip_kwargs(name):
    kw = dict(PIP[name]["kw"])
    if "ref" in kw:
        kw["ref"] = resolve_ref(kw["ref"])
    return kw


# ---- the model --------------------------------------------------------------------------------------------------------------------------------
def model_piptrack(S, *, sr=SR, n_fft=2048, fmin=150.0, fmax=4000.0, threshold=0.1, ref=None):
    """``piptrack(S=S)`` of the reference in NumPy, in the dtype of ``|S|``; the stencil is written out per element range."""
    S = np.asarray(S)
    if n_fft is None or n_fft // 2 + 1 != S.shape[-2]:
        n_fft = 2 * (S.shape[-2] - 1)
    if np.iscomplexobj(S) or S.min() < 0:
        S = np.abs(S)
    fmin = np.maximum(fmin, 0)
    fmax = np.minimum(fmax, float(sr) / 2)
    freqs = np.fft.rfftfreq(n=n_fft, d=1.0 / sr)
    x = np.moveaxis(S, -2, 0)  # bins first
    two, half = S.dtype.type(2), S.dtype.type(0.5)
    avg = np.empty_like(x)
    avg[1:-1] = (x[2:] - x[:-2]) / two
    avg[0], avg[-1] = x[1] - x[0], x[-1] - x[-2]
    shift = np.zeros_like(x)
    if x.shape[0] > 2:
        a = x[2:] + x[:-2] - two * x[1:-1]
        b = (x[2:] - x[:-2]) / two
        with np.errstate(divide="ignore", invalid="ignore"):
            shift[1:-1] = np.where(np.abs(b) >= np.abs(a), 0, -b / a)
    dskew = half * avg * shift
    mask = (fmin <= freqs) & (freqs < fmax)
    if ref is None:
        ref = np.max
    ref_value = threshold * ref(S, axis=-2) if callable(ref) else np.abs(ref)
    if callable(ref):
        ref_value = np.moveaxis(np.expand_dims(ref_value, -2), -2, 0)
    xt = x * (x > ref_value)
    lm = np.zeros(x.shape, dtype=bool)
    lm[1:-1] = (xt[1:-1] > xt[:-2]) & (xt[1:-1] >= xt[2:])
    lm[-1] = xt[-1] > xt[-2]
    peak = lm & mask.reshape((-1,) + (1,) * (x.ndim - 1))
    idx = np.nonzero(peak)
    pitches, mags = np.zeros_like(x), np.zeros_like(x)
    pitches[idx] = (idx[0] + shift[idx]) * float(sr) / n_fft
    mags[idx] = x[idx] + dskew[idx]
    return np.moveaxis(pitches, 0, -2), np.moveaxis(mags, 0, -2)


def tuning_edges(resolution):
    return np.linspace(-0.5, 0.5, int(np.ceil(1.0 / resolution)) + 1)


def model_residual(frequencies, bins_per_octave=12):
    f = np.atleast_1d(frequencies)
    f = f[f > 0]
    r = np.mod(bins_per_octave * np.log2(f / (440.0 / 16)), 1.0)
    r[r >= 0.5] -= 1.0
    return r


def model_pitch_tuning(frequencies, resolution=0.01, bins_per_octave=12):
    """-> (tuning, counts): ``pitch_tuning`` of the reference in the dtype of ``frequencies`` (no warning; 0.0 for an empty set)."""
    edges = tuning_edges(resolution)
    r = model_residual(frequencies, bins_per_octave)
    counts = np.histogram(r, edges)[0]
    return (float(edges[np.argmax(counts)]) if r.size else 0.0), counts


def model_select(pitches, mags):
    """The frequencies ``estimate_tuning`` hands to ``pitch_tuning``, and the threshold."""
    keep = pitches > 0
    thr = np.median(mags[keep]) if keep.any() else 0.0
    return pitches[(mags >= thr) & keep], thr


def model_estimate_tuning(S, resolution=0.01, bins_per_octave=12, **kw):
    pitches, mags = model_piptrack(S, **kw)
    return model_pitch_tuning(model_select(pitches, mags)[0], resolution, bins_per_octave)


def certify_tuning(S, resolution=0.01, bins_per_octave=12, **kw):
    """Why ``estimate_tuning(S=S)`` is NOT settled beyond rounding -- an empty list certifies the case: (1) the order statistics of the peaks'
    magnitudes next to the median cut are more than 16 ulp of the dtype apart, (2) no selected peak's float64 residual lies within 1e-4 of a
    histogram edge (the float32 log2 error at these magnitudes is about 1e-5), (3) the winning bin leads every other by at least 3 counts."""
    S = np.asarray(S)
    real = np.abs(S).dtype
    pitches, mags = model_piptrack(S, **kw)
    keep = pitches > 0
    why = []
    if not keep.any():
        return ["no peaks"]
    m = np.sort(mags[keep])
    n = m.size
    k1, k2 = (n - 1) // 2, n // 2
    near = m[max(k1 - 1, 0) : k2 + 2].astype(np.float64)
    gaps = np.diff(near)
    if gaps.size and gaps.min() <= 16 * np.spacing(np.abs(near).max().astype(real)):
        why.append(f"magnitudes at the median cut {near.tolist()} are within 16 ulp")
    chosen, _ = model_select(pitches, mags)
    r = model_residual(chosen.astype(np.float64), bins_per_octave)
    edges = tuning_edges(resolution)
    gap = np.abs(r[:, None] - edges[None, :]).min() if r.size else 1.0
    if gap <= 1e-4:
        why.append(f"a residual lies {gap:.2e} from a histogram edge")
    counts = np.sort(np.histogram(r, edges)[0])
    if counts.size > 1 and counts[-1] - counts[-2] < 3:
        why.append(f"the winning bin leads by {counts[-1] - counts[-2]}")
    return why


# ---- estimate_tuning cases ------------------------------------------------------------------------------------------------------------------
# Slowly decaying tones (so that no two frames' magnitudes tie), a few harmonics each, all detuned by `tuning` bins of `bins_per_octave`; 2 channels where `channels` says so.
TUNE_N_FFT = 2048
TUNING = {
    "r05_b12": dict(tuning=0.125, resolution=0.05, bins_per_octave=12, midi=(79, 84, 88, 91), seconds=0.6),
    "r05_b12_neg": dict(tuning=-0.275, resolution=0.05, bins_per_octave=12, midi=(81, 85, 90), seconds=0.6),
    "r03_b12": dict(tuning=0.2, resolution=0.03, bins_per_octave=12, midi=(84, 88, 91), seconds=0.6),
    "r01_b12": dict(tuning=0.115, resolution=0.01, bins_per_octave=12, midi=(96, 100), seconds=0.7),
    "r05_b36": dict(tuning=0.075, resolution=0.05, bins_per_octave=36, midi=(84, 88, 91), seconds=0.6),
    "r05_b12_2ch": dict(tuning=0.325, resolution=0.05, bins_per_octave=12, midi=(79, 86, 93), seconds=0.5, channels=2),
    "r05_b12_odd": dict(tuning=-0.125, resolution=0.05, bins_per_octave=12, midi=(84, 90, 97), seconds=0.58),  # 5 partials x 25 frames: an odd peak count
}
for _i, _c in enumerate(TUNING.values()):
    _c.setdefault("channels", 1)
    _c.setdefault("seed", 7000 + _i)


def tuning_signal(name):
    """float32 audio of a tuning case: (n,) or (channels, n)."""
    c = TUNING[name]
    rng = np.random.default_rng(c["seed"])
    n = int(round(c["seconds"] * SR))
    t = np.arange(n) / SR
    chans = []
    for ch in range(c["channels"]):
        y = np.zeros(n)
        for m in c["midi"]:
            f0 = 440.0 * 2.0 ** ((m - 69 + (12.0 / c["bins_per_octave"]) * c["tuning"]) / 12.0)
            for h, amp in ((1, 1.0), (2, 0.5)):
                if f0 * h < 3900:
                    y += amp * (0.8 + 0.4 * rng.random()) * np.exp(-(0.5 + 1.5 * rng.random()) * t) * np.sin(2 * np.pi * f0 * h * t + 2 * np.pi * rng.random())
        chans.append(y / np.abs(y).max() * 0.5)
    y = np.stack(chans) if c["channels"] > 1 else chans[0]
    return y.astype(np.float32)


def tuning_kwargs(name):
    c = TUNING[name]
    return dict(sr=SR, n_fft=TUNE_N_FFT, resolution=c["resolution"], bins_per_octave=c["bins_per_octave"])


def host_magnitudes(y, n_fft=TUNE_N_FFT, hop=None):
    """|stft(y)| in float64 arithmetic, rounded to float32: centred, zero-padded, periodic Hann -- the (..., 1 + n_fft // 2, n_frames) input of
    the ``S=`` cases (any magnitude array serves there; the reference sees the same bits)."""
    hop = n_fft // 4 if hop is None else hop
    y = np.asarray(y, dtype=np.float64)
    pad = [(0, 0)] * (y.ndim - 1) + [(n_fft // 2, n_fft // 2)]
    yp = np.pad(y, pad)
    n_frames = 1 + (yp.shape[-1] - n_fft) // hop
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    idx = np.arange(n_fft)[None, :] + hop * np.arange(n_frames)[:, None]
    frames = yp[..., idx] * win
    return np.swapaxes(np.abs(np.fft.rfft(frames, axis=-1)), -1, -2).astype(np.float32)


# ---- pitch_tuning cases ---------------------------------------------------------------------------------------------------------------------
def cqt_table(n_bins=24, fmin=55.0, tuning=0.25, bins_per_octave=12):
    """``cqt_frequencies(n_bins, fmin, tuning)`` (``core/convert.py``: fmin * 2 ** ((tuning + k) / bins_per_octave))."""
    return 2.0 ** (tuning / bins_per_octave) * fmin * 2.0 ** (np.arange(n_bins, dtype=np.float64) / bins_per_octave)


def _fold_list():
    # bins_per_octave = 0.5 and 27.5 * 2 ** k make every step exact: residual 0.5 k mod 1 is 0.5 for odd k -- the ">= 0.5" fold takes it to
    # -0.5, the first bin -- and 0 for even k.  (After the fold a residual lies in [-0.5, 0.5): the histogram's closed last edge is out of
    # reach of pitch_tuning; the host suite tests it on the bin search directly.)
    return 27.5 * 2.0 ** np.array([1.0, 3.0, 5.0, 2.0, 4.0])


PITCH_TUNING = {
    "cqt_quarter": dict(freqs=cqt_table(), kw={}),
    # (in float32 a table at exactly 0.25 puts every residual within 1.2e-7 of the edge 0.25 -- inside the rounding of log2f, so the bin is
    #  not determined; the float32 table sits mid-bin instead)
    "cqt_quarter_f32": dict(freqs=cqt_table(tuning=0.255).astype(np.float32), kw={}),
    "trimmed": dict(freqs=np.concatenate([[0.0, -440.0, -1.0], cqt_table(36, 65.0, -0.3), [0.0]]), kw=dict(resolution=0.05)),
    "fold": dict(freqs=_fold_list(), kw=dict(resolution=0.1, bins_per_octave=0.5)),
    "fold_f32": dict(freqs=_fold_list().astype(np.float32), kw=dict(resolution=0.1, bins_per_octave=0.5)),
    "b36": dict(freqs=cqt_table(72, 32.7, 0.1, 36), kw=dict(resolution=0.05, bins_per_octave=36)),
    "many": dict(freqs=np.tile(cqt_table(60, 55.0, -0.15), 200), kw=dict(resolution=0.02)),  # several segments of the plain walk
    "fine": dict(freqs=cqt_table(48, 55.0, 0.2305), kw=dict(resolution=0.0002)),  # 5000 bins: beyond the staged histogram
    "empty": dict(freqs=np.zeros(0), kw={}),
    "nothing_positive": dict(freqs=np.array([0.0, -3.0, 0.0]), kw={}),
}


def pitch_tuning_margin(name):
    """The distance of the case's float64 residuals from the nearest histogram edge (1.0 for an empty set)."""
    c = PITCH_TUNING[name]
    r = model_residual(np.asarray(c["freqs"], dtype=np.float64), c["kw"].get("bins_per_octave", 12))
    return float(np.abs(r[:, None] - tuning_edges(c["kw"].get("resolution", 0.01))[None, :]).min()) if r.size else 1.0


def ulp_distance(got, want):
    """The largest |got - want| in units of the last place of ``want``'s dtype at ``want``'s magnitude."""
    got, want = np.asarray(got), np.asarray(want)
    if want.size == 0:
        return 0.0
    unit = np.spacing(np.abs(want).astype(want.dtype)).astype(np.float64)
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / unit).max())
