"""The edge-case table of the rhythm chain (tempogram / tempo, beat tracker, onset strength), shared by tests/test_rhythm_oracle.py,
tests/test_rhythm_edges_host.py and tests/test_rhythm_edges_gpu.py.  Inputs are tiny and come from fixed seeds; the reference's results for
the part of the table that pins the oracle are in tests/golden/rhythm_edges.npz (scripts/make_rhythm_edges_golden.py), which stores results
and input checksums only."""
import json
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rhythm_edges.npz")

# ---- the tempogram kernel's geometry, restated from librosa_amd/csrc/lra_rhythm.h and lra_mixed_sizes.h ------------------------------------
SIZES = (160, 200, 240, 320, 400, 480, 600, 640, 720, 800, 882, 960, 1000, 1200, 1280, 1440, 1600, 1764, 1920, 2000, 2400, 2646, 3200, 3528, 4800)
WRITE, SUM, ARGMAX = 0, 1, 2
GROUP, RED, LDS_MAX = 16, 64, 160 * 1024


def transform_length(W):
    """The smallest transform size that holds 2 W - 1 samples, or 0: the direct kernel."""
    return min((N for N in SIZES if N >= 2 * W - 1), default=0)


def chunk_frames(N):
    fc = GROUP
    while fc > 1 and fc * 2 * (N // 2) * 16 > 48 * 1024:
        fc //= 2
    return fc


def lds_total(W, mode, tile):
    """lds_layout(transform_length(W), W, mode, tile).total in bytes."""
    N = transform_length(W)
    fc = chunk_frames(N) if N else 1
    core = (2 * fc * (N // 2) + N // 2) * 16 if N else 2 * W * 8
    extra = W * 8 if mode == SUM else (W * GROUP * 8 if mode == WRITE and tile else 0)
    return core + fc * RED * 8 + fc * RED * 4 + fc * 8 + extra


def first_refused(mode):
    """The smallest win_length whose layout (without the tile) exceeds the LDS of a workgroup."""
    W = 2401
    while lds_total(W, mode, False) <= LDS_MAX:
        W += 1
    return W


def _seed(name):
    return zlib.crc32(name.encode())


# ---- tempogram / tempo -------------------------------------------------------------------------------------------------------------------------
def _tg(name, W, n, dtype="float32", center=True, norm="inf", batch=None, modes=(WRITE,)):
    return dict(name=name, W=W, n=n, dtype=dtype, center=center, norm=norm, batch=batch, modes=tuple(modes))


def _tg_cases():
    cases = []
    all_modes = (WRITE, SUM, ARGMAX)
    largest = [(N + 1) // 2 for N in SIZES]
    for i, (N, W) in enumerate(zip(SIZES, largest)):
        assert transform_length(W) == N and (W + 1 > largest[-1] or transform_length(W + 1) != N)
        cases.append(_tg(f"n{N}_w{W}", W, 19 + (7 * i) % 19, modes=all_modes))
    for N, prev in zip(SIZES[-6:], largest[-7:-1]):  # the six largest sizes: also the smallest window that maps to them
        assert transform_length(prev + 1) == N
        cases.append(_tg(f"n{N}_w{prev + 1}", prev + 1, 19 + (prev % 19), modes=all_modes))
    for W in (2401, 2756):  # beyond the size list: the direct O(W^2) kernel
        assert transform_length(W) == 0
        cases.append(_tg(f"direct_w{W}", W, 19 + W % 7, modes=all_modes))
    for W in (1, 2, 3):
        cases.append(_tg(f"w{W}", W, 21 + W, modes=all_modes))
    # the WRITE epilogue with and without the staged LDS tile: the boundary lies inside N = 1920
    assert transform_length(900) == 1920 and lds_total(900, WRITE, True) <= LDS_MAX < lds_total(960, WRITE, True)
    cases.append(_tg("tile_w900", 900, 23))
    cases.append(_tg("notile_w960_33", 960, 33))
    for W in (80, 441, 1600):  # a small, a middle (radix 7) and a large size
        for n in (1, 15, 16, 17, 33):  # group (16 frames) and chunk remainders
            cases.append(_tg(f"w{W}_frames{n}", W, n))
        cases.append(_tg(f"w{W}_nocenter", W, W, center=False))
        cases.append(_tg(f"w{W}_f64", W, 20, dtype="float64", modes=all_modes))
        for norm in ("1", "2", "none"):
            cases.append(_tg(f"w{W}_norm_{norm}", W, 18, norm=norm))
        cases.append(_tg(f"w{W}_batch3", W, 19, batch=3, modes=all_modes))
    return {c["name"]: c for c in cases}


TG_CASES = _tg_cases()
NORMS = {"inf": np.inf, "1": 1, "2": 2, "none": None}


def tg_envelope(case):
    """Noise plus a pulse every few frames, in the case's dtype ((batch, n) or (n,))."""
    rng = np.random.default_rng(_seed("tg:" + case["name"]))
    shape = (case["n"],) if case["batch"] is None else (case["batch"], case["n"])
    env = np.abs(rng.standard_normal(shape))
    env[..., :: 5 + case["W"] % 4] += 3.0
    return env.astype(case["dtype"])


def tempo_kwargs(case):
    """feature.tempo arguments whose autocorrelation window is the case's W frames: ac_size 1 s at ``sr = W`` frames per second."""
    return dict(sr=case["W"], hop_length=1, ac_size=1.0)


# ---- beat tracker ------------------------------------------------------------------------------------------------------------------------------
FRAME_RATE = 100.0
BEAT_KW = dict(sr=100, hop_length=1)  # beat_track's frame rate: sr / hop_length
BEAT_ROWS = ((63, 3), (64, 5), (65, 7), (257, 2), (300, 9), (700, 41), (2049, 22), (2600, 22), (2600, 1024), (2600, 1025), (130, 20.5), (130, 21.5), (5000, 60))


def bpm_of(fpb):
    """A tempo whose ``FRAME_RATE * 60 / bpm`` is exactly ``fpb`` in float64 (so that x.5 rounds half to even, not by a rounding error)."""
    b = 6000.0 / fpb
    for cand in (b, np.nextafter(b, 0), np.nextafter(b, np.inf), np.nextafter(np.nextafter(b, 0), 0), np.nextafter(np.nextafter(b, np.inf), np.inf)):
        if FRAME_RATE * 60.0 / cand == fpb:
            return float(cand)
    raise AssertionError(f"no float64 tempo gives exactly {fpb} frames per beat")


def _beat(name, rows, dtype="float32", tightness=100, trim=True, per_frame=False, seed=0):
    return dict(name=name, rows=rows, dtype=dtype, tightness=tightness, trim=trim, per_frame=per_frame, seed=seed)


def _beat_cases():
    cases = [_beat(f"n{n}_fpb{str(f).replace('.', 'p')}", [(n, f)]) for n, f in BEAT_ROWS]
    cases.append(_beat("f64", [(300, 9)], dtype="float64"))
    cases.append(_beat("trim_false", [(700, 41)], trim=False))
    cases.append(_beat("tight_10", [(700, 41)], tightness=10))
    cases.append(_beat("tight_1e4", [(700, 41)], tightness=1e4))
    cases.append(_beat("per_frame", [(2600, None)], per_frame=True))
    cases.append(_beat("batch5", [(300, 5), (300, 9), (300, 0), (300, 22), (300, 41)]))  # fpb 0: an all-zero row between live rows
    return {c["name"]: c for c in cases}


BEAT_CASES = _beat_cases()
# a seed that does not certify (oracle.certify at the fixture's radius) is replaced here
BEAT_SEEDS = {}
RADIUS, DRAWS = 1e-5, 8


def per_frame_fpb(n):
    """Frames per beat that move between 4 and 1100 inside one row."""
    f = np.full(n, 4.0)
    f[n // 4 : 3 * n // 4] = 1100.0
    f[3 * n // 4 : 7 * n // 8] = 37.0
    return f


def beat_inputs(case):
    """-> (env, bpm): env (n,) or (rows, n); bpm a float, (rows,) or per frame (n,)."""
    rng = np.random.default_rng(_seed("beat:" + case["name"]) + BEAT_SEEDS.get(case["name"], case["seed"]))
    envs, bpms = [], []
    for n, f in case["rows"]:
        if case["per_frame"]:
            fpb = per_frame_fpb(n)
            env = 0.3 * np.abs(rng.standard_normal(n))
            t = 0
            while t < n:
                env[t] += 3.0
                t += int(fpb[t])
            envs.append(env)
            lut = {v: bpm_of(v) for v in np.unique(fpb)}
            bpms.append(np.array([lut[v] for v in fpb]))
        elif f == 0:
            envs.append(np.zeros(n))
            bpms.append(120.0)
        else:
            env = 0.3 * np.abs(rng.standard_normal(n))
            env[rng.integers(0, int(np.round(f))) :: int(np.round(f))] += 3.0
            envs.append(env)
            bpms.append(bpm_of(float(f)))
    if len(envs) == 1:
        return envs[0].astype(case["dtype"]), (bpms[0] if case["per_frame"] else float(bpms[0]))
    return np.stack(envs).astype(case["dtype"]), np.array(bpms)


# ---- onset strength (from S=, so that the band count is free) ----------------------------------------------------------------------------------
def _on(name, bands, frames, dtype="float32", agg="median", channels=None, lag=1, max_size=1, detrend=False, batch=None, ties=False, nan=False):
    return dict(name=name, bands=bands, frames=frames, dtype=dtype, agg=agg, channels=channels, lag=lag, max_size=max_size, detrend=detrend, batch=batch, ties=ties, nan=nan)


def _onset_cases():
    cases = []
    # median over one channel of every band: 64 down to 1 threads per workgroup, the last at exactly 160 KiB of LDS
    for i, bands in enumerate((255, 256, 257, 513, 1025, 2049, 8192, 8193, 40960)):
        cases.append(_on(f"median_f32_{bands}", bands, (70, 66, 65, 33, 17, 9, 5, 4, 3)[i]))
    for bands, frames in ((128, 67), (129, 34), (4097, 3)):
        cases.append(_on(f"median_f64_{bands}", bands, frames, dtype="float64"))
    cases.append(_on("median_slices", 1025, 19, channels=[[0, 1025, 2], [100, 901, 1], [1024, 0, -3], [7, 8, 1]]))  # stepped, overlapping, reversed, one band
    cases.append(_on("median_bounds", 300, 70, channels=[0, 3, 260, 300]))  # integer boundaries: 3, 257 and 40 bands
    cases.append(_on("median_ties", 257, 40, ties=True))
    cases.append(_on("median_ties_even", 256, 40, ties=True))
    cases.append(_on("median_nan", 513, 12, nan=True))
    for agg in ("mean", "sum", "max", "min", "false"):  # the flux kernel's 256-frame tile and its remainder
        for frames in (255, 256, 257, 513):
            cases.append(_on(f"{agg}_{frames}", 5, frames, agg=agg))
    for ms in (2, 7, 13):  # 13 = 2 * bands + 3: wider than the reflect period
        cases.append(_on(f"max_size_{ms}", 5, 30, agg="mean", max_size=ms))
        cases.append(_on(f"max_size_{ms}_median", 5, 30, max_size=ms))
    cases.append(_on("lag_frames_minus_1", 6, 9, agg="mean", lag=8))
    cases.append(_on("lag_ge_frames", 6, 9, agg="mean", lag=11))
    for rows in (15, 16, 17):  # the detrend tile: 16 rows by 64 frames
        for frames in (63, 64, 65, 129):
            cases.append(_on(f"detrend_{rows}x{frames}", 4, frames, agg="mean", detrend=True, batch=rows))
    return {c["name"]: c for c in cases}


ONSET_CASES = _onset_cases()
ONSET_REFUSED_BANDS = 40961  # one float32 band more than 160 KiB of LDS hold
AGGREGATES = dict(mean=np.mean, sum=np.sum, max=np.max, min=np.min, median=np.median, false=False)
SELECTIONS = ("max", "min", "false")  # and medians of odd-sized channels: bit-equal to NumPy in the same dtype


def onset_channels(case):
    ch = case["channels"]
    if ch is None or not isinstance(ch[0], list):
        return ch
    return [slice(a, b, s) for a, b, s in ch]


def onset_input(case):
    rng = np.random.default_rng(_seed("onset:" + case["name"]))
    shape = (case["bands"], case["frames"]) if case["batch"] is None else (case["batch"], case["bands"], case["frames"])
    S = rng.standard_normal(shape) * 4.0
    if case["ties"]:
        S = np.round(S)
    S = S.astype(case["dtype"])
    if case["nan"]:
        S[case["bands"] // 3, case["frames"] // 2] = np.nan
    return S


def onset_kwargs(case):
    return dict(lag=case["lag"], max_size=case["max_size"], detrend=case["detrend"], aggregate=AGGREGATES[case["agg"]], channels=onset_channels(case))


def check_onset(case, got, S, run_plain):
    """The bounds of the edge table's onset cases; ``run_plain``: the same call without ``detrend`` (the detrended rows are compared with
    the float64 lfilter of the implementation's own envelope)."""
    import rhythm_oracle as O

    kw = onset_kwargs(case)
    want = O.onset_multi(S, **kw)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    scale = max(float(np.max(np.abs(want[ok]))), 1e-30) if ok.any() else 1.0
    if case["detrend"]:
        import scipy.signal

        own = run_plain()
        assert own.dtype == S.dtype
        ref = scipy.signal.lfilter(np.array([1.0, -1.0]), np.array([1.0, -0.99]), own.astype(np.float64), axis=-1)
        assert np.max(np.abs(got - ref)) <= 1e-9 * max(float(np.max(np.abs(ref))), 1e-30)
        plain = O.onset_multi(S.astype(np.float64), **dict(kw, detrend=False))
        assert np.all(np.abs(own - plain) - 1e-5 * np.abs(plain) <= 1e-5 * np.max(np.abs(plain)))
        return
    sizes = [len(np.arange(case["bands"])[s]) for s in O.channel_slices(kw["channels"], case["bands"])]
    if case["agg"] in SELECTIONS or (case["agg"] == "median" and all(n % 2 for n in sizes)):
        assert np.array_equal(got, want, equal_nan=True)  # a selection: the same bits as NumPy in the same dtype
        return
    wide = O.onset_multi(S.astype(np.float64), **kw)  # sums, means, even-count medians: against float64
    d = np.abs(got[ok].astype(np.float64) - wide[ok])
    if case["dtype"] == "float64":
        assert d.max(initial=0.0) <= 1e-9 * scale
    else:
        assert np.all(d - 1e-5 * np.abs(wide[ok]) <= 1e-5 * scale)


# ---- the fixture -------------------------------------------------------------------------------------------------------------------------------
# what the fixture pins: where the three older fixtures do not reach
GOLDEN_TG = ("w1", "w2", "w3", "n882_w441", "direct_w2401", "w441_f64", "w80_nocenter", "w441_norm_1", "w441_norm_2", "w441_norm_none")
GOLDEN_BEAT = tuple(BEAT_CASES)
GOLDEN_ONSET = ("max_size_2", "max_size_7", "max_size_13", "max_size_13_median", "lag_frames_minus_1", "lag_ge_frames", "median_slices", "median_bounds", "median_ties_even",
                "median_nan", "detrend_17x65", "false_257")
GOLDEN_COLS = 3


def golden_cols(n):
    return np.unique([0, n // 2, n - 1]).astype(np.int64)


def checksum(a):
    return float(np.nansum(np.asarray(a, dtype=np.float64)))


def load():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["params"]))
