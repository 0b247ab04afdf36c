"""Cases for the constant-Q octave kernels (csrc/lra_mixed.h: cqt_octave_body as mixed_cqt_kernel and mixed_cqt_multi_kernel; csrc/lra_cqt.h:
cqt_project_kernel), shared by the host test on the simulator (tests/test_cqt_octave_host.py) and the device test (tests/test_cqt_octave_gpu.py),
and their plain reference.  Imports neither the native library nor the simulator.

DIRECT cases drive one octave launch: one family per frame length of the library's list and precision, each a list of runs (`family`).
WHOLE cases are cqt / vqt calls whose plans (constantq._plan) reach every frame length of the list and one beyond it (`WHOLE`).

The bar of a direct run (`build`): for every used row r, max |got - ref| over clips and frames <= bar x max |ref| of that row, where
  bar_f32 = 4 x the worst per-row ratio of the plain working-precision computation of the same run against the float64 reference
            (scipy.fft.rfft of the float32 frames, complex64 products summed in CSR order; 4: another summation order inside the transform, fused multiply-adds),
  bar_f64 = bar_f32 x 2**-29 (the same operation sequence in both types),
neither above the whole-transform bars (2e-5, 1e-11).
"""
import os
import re

import numpy as np
import scipy.fft

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "librosa_amd", "csrc")
PAD_MODES = ("constant", "reflect", "edge", "symmetric")
DTYPES = (np.float32, np.float64)
BATCH = 3
ROW_ENTRIES = (0, 1, 7, 8, 9, 15, 16, 17, 23, 40, 3, 64)   # per row, each capped at n_fft // 2 + 1: no entry, one, both sides of one, two and three batches of eight, five and eight whole batches
OFFSETS = dict(row0=1, n_rows=10, bin0=3, n_total=18)       # the octave's rows and where they land in the stacked result
OFFSETS_ALL = dict(row0=0, n_rows=12, bin0=3, n_total=20)   # every row, the empty one and the longest included
WHOLE_BAR = {np.dtype(np.float32): 2e-5, np.dtype(np.float64): 1e-11}


def sizes():
    """The fused octave kernel's frame lengths, read from the library's own list (csrc/lra_mixed_sizes.h: LRA_CQT_SIZES)."""
    text = open(os.path.join(CSRC, "lra_mixed_sizes.h")).read()
    line = re.search(r"^#define LRA_CQT_SIZES\(X\)(.*)$", text, re.M).group(1)
    found = tuple(int(v) for v in re.findall(r"X\((\d+)\)", line))
    assert found and re.sub(r"X\(\d+\)|\s", "", line) == "", line
    return found


SIZES = sizes()
SHORT_SIZES = tuple(s for s in (256, 4096) if s in SIZES)   # the families that also carry signals shorter than the padding
INSTANCES = [(n_fft, dt) for n_fft in SIZES for dt in DTYPES]


def instance_id(inst):
    return f"{inst[0]}-{np.dtype(inst[1]).name}"


# ---- the synthetic basis ------------------------------------------------------------------------------------------------------------------
def rows(n_fft, dtype):
    """CSR (row_ptr, col, val) of the 12 synthetic rows and sqrt_len per row.  Columns sorted; bin 0 and bin n_fft // 2 each occur in a used row; values
    random complex, scaled by 1 / sqrt(entries)."""
    n_bins = n_fft // 2 + 1
    cplx = np.complex128 if np.dtype(dtype) == np.float64 else np.complex64
    rng = np.random.default_rng(1000 + n_fft)
    row_ptr, col, val = [0], [], []
    for r, want in enumerate(ROW_ENTRIES):
        k = min(want, n_bins)
        c = np.sort(rng.choice(n_bins, size=k, replace=False))
        if r == 2 and 0 not in c:
            c[0] = 0
        if r == 4 and n_bins - 1 not in c:
            c[-1] = n_bins - 1
        v = (rng.standard_normal(k) + 1j * rng.standard_normal(k)) / np.sqrt(max(k, 1))
        col.extend(c.tolist())
        val.extend(v.tolist())
        row_ptr.append(len(col))
    row_ptr, col, val = np.array(row_ptr, np.int32), np.array(col, np.int32), np.array(val, np.complex128).astype(cplx)
    sqrt_len = np.sqrt(rng.random(len(ROW_ENTRIES)) * 100 + 1)
    counts = np.diff(row_ptr)
    assert list(counts) == [min(w, n_bins) for w in ROW_ENTRIES] and all(np.all(np.diff(col[a:b]) > 0) for a, b in zip(row_ptr[:-1], row_ptr[1:]))
    used = col[row_ptr[OFFSETS["row0"]] : row_ptr[OFFSETS["row0"] + OFFSETS["n_rows"]]]
    assert 0 in used and n_bins - 1 in used
    return row_ptr, col, val, sqrt_len


# ---- the runs of a family -------------------------------------------------------------------------------------------------------------------
def full_frames(n, hop):
    return 1 + n // hop


def _pick_hop(base, odd):
    """(n, hop) of the wanted parity (both odd or both even), n as close to `base` as there is one, hop the largest, such that the frame count is at least 17 and
    a multiple of none of 2 .. 8: more than two groups of the largest frames-per-group (8) and a partial last group whatever the instance's F is."""
    for step in range(0, 12, 2):
        for n in (base + step, base - step):
            for hop in range(n // 16, 0, -1):
                count = full_frames(n, hop)
                if (hop % 2 == 1) == odd and count >= 17 and all(count % f for f in range(2, 9)):
                    return n, hop
    raise AssertionError((base, odd))


def family(inst):
    """The runs of one (n_fft, dtype) instance: dicts of n, hop, pad_mode, n_frames, scaled and the row offsets.  Signals: `signal(inst, run)`."""
    n_fft, _ = inst
    (n_odd, h_odd), (n_even, h_even) = _pick_hop(2 * n_fft + 11, True), _pick_hop(2 * n_fft + 12, False)
    f_odd, f_even = full_frames(n_odd, h_odd), full_frames(n_even, h_even)

    def run(name, n, hop, pad_mode, n_frames, scaled, off=OFFSETS):
        return dict(name=name, n_fft=n_fft, n=n, hop=hop, pad_mode=pad_mode, n_frames=n_frames, scaled=scaled, **off)

    runs = [run("odd-reflect-scaled", n_odd, h_odd, "reflect", f_odd, True),
            run("odd-symmetric", n_odd, h_odd, "symmetric", f_odd, False),
            run("even-constant-scaled", n_even, h_even, "constant", f_even, True),
            run("even-edge", n_even, h_even, "edge", f_even, False),
            run("odd-constant-one-frame", n_odd, h_odd, "constant", 1, True),
            run("even-reflect-fewer-frames", n_even, h_even, "reflect", f_even - 2, True),
            run("odd-edge-all-rows-scaled", n_odd, h_odd, "edge", f_odd, True, OFFSETS_ALL),
            run("even-symmetric-all-rows", n_even, h_even, "symmetric", f_even, False, OFFSETS_ALL)]
    if n_fft in SHORT_SIZES:   # shorter than the padding: fetch's repeated reflection; one sample: its n == 1 branch
        for n in (n_fft // 2 - 3, 1):
            hop = max(1, n // 4) | 1
            for pad_mode in ("reflect", "symmetric", "edge"):
                runs.append(run(f"short{n}-{pad_mode}", n, hop, pad_mode, full_frames(n, hop), True))
    check_family(inst, runs)
    return runs


def check_family(inst, runs, F=None):
    """What a family must cover; with F (the instance's frames per workgroup, from the library through the simulator) also the group geometry."""
    n_fft, _ = inst
    pad = n_fft // 2
    main = [r for r in runs if not r["name"].startswith("short")]
    assert {r["pad_mode"] for r in main} == set(PAD_MODES) and {r["scaled"] for r in main} == {True, False}
    odd = [r for r in main if r["hop"] % 2 == 1]
    even = [r for r in main if r["hop"] % 2 == 0]
    assert odd and even and all(r["n"] % 2 == 1 for r in odd) and all(r["n"] % 2 == 0 for r in even)
    assert any(r["n_frames"] == 1 for r in main) and any(1 < r["n_frames"] < full_frames(r["n"], r["hop"]) for r in main)
    assert all(abs(r["n"] - (2 * n_fft + 11)) <= 11 for r in main)   # about 2 n_fft + 11 samples
    assert any((r["row0"], r["n_rows"], r["bin0"], r["n_total"]) == (1, 10, 3, 18) for r in odd) and any((r["row0"], r["n_rows"], r["bin0"], r["n_total"]) == (1, 10, 3, 18) for r in even)
    assert any(r["row0"] == 0 and r["n_rows"] == len(ROW_ENTRIES) for r in main)   # the empty row and the longest are used somewhere
    for r in runs:
        assert 1 <= r["n_frames"] <= full_frames(r["n"], r["hop"])
    for r in main:
        if r["n_frames"] == full_frames(r["n"], r["hop"]):
            last = (r["n_frames"] - 1) * r["hop"] - pad
            assert -pad < 0 and last + n_fft - 1 > r["n"] - 1, r    # the first frame reaches before sample 0, the last one past sample n - 1
    for r in odd:
        if r["n_frames"] == full_frames(r["n"], r["hop"]):        # a sample pair (n - 1, n) that straddles the signal's end
            assert any((r["n"] - 1 - (f * r["hop"] - pad)) % 2 == 0 and 0 <= r["n"] - 1 - (f * r["hop"] - pad) <= n_fft - 2 for f in range(r["n_frames"])), r
    if n_fft in SHORT_SIZES:
        short = [r for r in runs if r["name"].startswith("short")]
        assert {(r["n"], r["pad_mode"]) for r in short} == {(n, m) for n in (n_fft // 2 - 3, 1) for m in ("reflect", "symmetric", "edge")}
    if F is not None:
        full = [r for r in main if r["n_frames"] == full_frames(r["n"], r["hop"])]
        assert {r["hop"] % 2 for r in full} == {0, 1}
        for r in full:
            assert r["n_frames"] > F and (F == 1 or r["n_frames"] % F != 0) and (F < 5 or r["n_frames"] >= 2 * F + 1), (r, F)


def signal(inst, run):
    """(BATCH, n) signal of a run in the instance's type; the same for every run of a family with the same n."""
    n_fft, dtype = inst
    rng = np.random.default_rng(7 * n_fft + run["n"])
    return rng.standard_normal((BATCH, run["n"])).astype(dtype)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def frames_of(y, n_fft, hop, pad_mode, n_frames):
    """np.pad + frames at `hop` (rectangular window): (batch, n_frames, n_fft), in y's type."""
    padded = np.pad(y, [(0, 0), (n_fft // 2, n_fft // 2)], mode=pad_mode)
    idx = np.arange(n_frames)[:, None] * hop + np.arange(n_fft)[None, :]
    return padded[:, idx]


def project_reference(D, row_ptr, col, val, sqrt_len, row0, n_rows, bin0, n_total):
    """The used rows' complex128 dot products with the bins of D (batch, n_frames, n_bins), divided by sqrt_len[r] where given (index 0 = row0), at columns
    bin0 .. bin0 + n_rows of a (batch, n_frames, n_total) array that is NaN elsewhere."""
    D = np.asarray(D, np.complex128)
    out = np.full(D.shape[:2] + (n_total,), np.nan + 1j * np.nan, dtype=np.complex128)
    for r in range(n_rows):
        a, b = row_ptr[row0 + r], row_ptr[row0 + r + 1]
        acc = D[:, :, col[a:b]] @ np.asarray(val[a:b], np.complex128)
        out[:, :, bin0 + r] = acc / sqrt_len[r] if sqrt_len is not None else acc
    return out


def project_plain_f32(D, row_ptr, col, val, sqrt_len, row0, n_rows):
    """The same projection in plain working precision: complex64 products summed in CSR order -> (batch, n_frames, n_rows)."""
    D, val = np.asarray(D, np.complex64), np.asarray(val, np.complex64)
    out = np.zeros(D.shape[:2] + (n_rows,), np.complex64)
    for r in range(n_rows):
        acc = np.zeros(D.shape[:2], np.complex64)
        for j in range(row_ptr[row0 + r], row_ptr[row0 + r + 1]):
            acc = acc + val[j] * D[:, :, col[j]]
        out[:, :, r] = (acc.astype(np.complex128) * (1.0 / sqrt_len[r])).astype(np.complex64) if sqrt_len is not None else acc
    return out


def reference(y, n_fft, hop, pad_mode, n_frames, row_ptr, col, val, sqrt_len, row0, n_rows, bin0, n_total):
    """Plain NumPy in float64: np.pad, frames at `hop` with a rectangular window, np.fft.rfft, then `project_reference`."""
    D = np.fft.rfft(frames_of(np.asarray(y, np.float64), n_fft, hop, pad_mode, n_frames), axis=-1)
    return project_reference(D, row_ptr, col, val, sqrt_len, row0, n_rows, bin0, n_total)


def plain_f32(y, n_fft, hop, pad_mode, n_frames, row_ptr, col, val, sqrt_len, row0, n_rows):
    """The same octave in plain working precision: scipy.fft.rfft of the float32 frames, then `project_plain_f32`."""
    D = scipy.fft.rfft(frames_of(np.asarray(y, np.float32), n_fft, hop, pad_mode, n_frames), axis=-1)
    assert D.dtype == np.complex64
    return project_plain_f32(D, row_ptr, col, val, sqrt_len, row0, n_rows)


def row_ratios(got, ref):
    """Per column: max |got - ref| over clips and frames / max |ref|; 0 where both are zero everywhere."""
    err = np.abs(got - ref).reshape(-1, ref.shape[-1]).max(axis=0)
    peak = np.abs(ref).reshape(-1, ref.shape[-1]).max(axis=0)
    return np.where(peak > 0, err / np.where(peak > 0, peak, 1), np.where(err > 0, np.inf, 0.0))


_BUILT = {}


def build(inst, run):
    """A run's inputs, reference and bar, computed once and left unchanged: dict(y, row_ptr, col, val, sqrt_len (used rows or None), ref, bar, plain_ratio)."""
    key = (inst[0], np.dtype(inst[1]).str, run["name"])
    if key in _BUILT:
        return _BUILT[key]
    n_fft, dtype = inst
    y = signal(inst, run)
    row_ptr, col, val, sqrt_all = rows(n_fft, dtype)
    row0, n_rows, bin0, n_total = run["row0"], run["n_rows"], run["bin0"], run["n_total"]
    sqrt_len = np.ascontiguousarray(sqrt_all[row0 : row0 + n_rows]) if run["scaled"] else None
    geom = (n_fft, run["hop"], run["pad_mode"], run["n_frames"])
    ref = reference(y, *geom, row_ptr, col, val, sqrt_len, row0, n_rows, bin0, n_total)
    # the bar: the float32 form of the same run (inputs rounded to float32) against ITS float64 reference
    y32, val32 = y.astype(np.float32), val.astype(np.complex64)
    ref32 = reference(y32, *geom, row_ptr, col, val32, sqrt_len, row0, n_rows, 0, n_rows)
    plain_ratio = float(row_ratios(plain_f32(y32, *geom, row_ptr, col, val32, sqrt_len, row0, n_rows), ref32).max())
    bar32 = min(4 * plain_ratio, WHOLE_BAR[np.dtype(np.float32)])
    bar = bar32 if np.dtype(dtype) == np.float32 else min(bar32 * 2.0**-29, WHOLE_BAR[np.dtype(np.float64)])
    assert np.isfinite(plain_ratio) and plain_ratio > 0
    c = dict(y=y, row_ptr=row_ptr, col=col, val=val, sqrt_len=sqrt_len, ref=ref, bar=bar, plain_ratio=plain_ratio)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _BUILT[key] = c
    return c


def compare(got, c, run):
    """(worst ratio over the used rows, message) of a (batch, n_frames, n_total) result against the run's reference; asserts nothing."""
    bin0, n_rows = run["bin0"], run["n_rows"]
    ratios = row_ratios(np.asarray(got)[:, :, bin0 : bin0 + n_rows].astype(np.complex128), c["ref"][:, :, bin0 : bin0 + n_rows])
    worst = float(ratios.max())
    return worst, f"n_fft {run['n_fft']} {run['name']}: worst row ratio {worst:.3g} (row {run['row0'] + int(ratios.argmax())}), bar {c['bar']:.3g}, plain float32 ratio {c['plain_ratio']:.3g}"


# ---- the projection kernel of the two-launch route, alone -----------------------------------------------------------------------------------
PROJECT_SIZES = (128, 8192)   # a frame length of the fused list and the first one beyond it
PROJECT_OFFSETS = ((37, 40, 20, 0, 12, True), (30, 12, 0, 0, 12, False), (37, 7, 0, 5, 7, True), (1, 30, 18, 0, 12, True))   # (n_frames, n_total, bin0, row0, n_rows, scaled): tests/test_hostsim.py, test_cqt_project_body


def build_project(n_fft, dtype):
    """Random D (2, 37, n_fft // 2 + 1) in the type's complex form, the synthetic rows, and per offset tuple the reference and the bar (as `build`: 4 x the plain
    float32 projection's worst per-row ratio, x 2**-29 in float64, capped by the whole-transform bars)."""
    key = ("project", n_fft, np.dtype(dtype).str)
    if key in _BUILT:
        return _BUILT[key]
    cplx = np.complex128 if np.dtype(dtype) == np.float64 else np.complex64
    rng = np.random.default_rng(12 + n_fft)
    n_bins = n_fft // 2 + 1
    D = (rng.standard_normal((2, 37, n_bins)) + 1j * rng.standard_normal((2, 37, n_bins))).astype(cplx)
    row_ptr, col, val, sqrt_all = rows(n_fft, dtype)
    D32, val32 = D.astype(np.complex64), val.astype(np.complex64)
    cases = []
    for n_frames, n_total, bin0, row0, n_rows, scaled in PROJECT_OFFSETS:
        sqrt_len = np.ascontiguousarray(sqrt_all[row0 : row0 + n_rows]) if scaled else None
        ref = project_reference(D[:, :n_frames], row_ptr, col, val, sqrt_len, row0, n_rows, bin0, n_total)
        ref32 = project_reference(D32[:, :n_frames], row_ptr, col, val32, sqrt_len, row0, n_rows, 0, n_rows)
        plain_ratio = float(row_ratios(project_plain_f32(D32[:, :n_frames], row_ptr, col, val32, sqrt_len, row0, n_rows), ref32).max())
        bar32 = min(4 * plain_ratio, WHOLE_BAR[np.dtype(np.float32)])
        bar = bar32 if np.dtype(dtype) == np.float32 else min(bar32 * 2.0**-29, WHOLE_BAR[np.dtype(np.float64)])
        assert np.isfinite(plain_ratio) and plain_ratio > 0
        cases.append(dict(n_fft=n_fft, name=f"project-{n_frames}-{n_total}-{bin0}-{row0}-{n_rows}", n_frames=n_frames, n_total=n_total, bin0=bin0, row0=row0, n_rows=n_rows, sqrt_len=sqrt_len, ref=ref,
                          bar=bar, plain_ratio=plain_ratio))
    c = dict(D=D, row_ptr=row_ptr, col=col, val=val, cases=cases)
    for a in (D, row_ptr, col, val):
        a.setflags(write=False)
    _BUILT[key] = c
    return c


# ---- whole transforms -----------------------------------------------------------------------------------------------------------------------
SR = 22050
# (name, function, keyword arguments, the octaves' frame lengths as constantq._plan gives them)
WHOLE = [("n32", "cqt", dict(filter_scale=0.125, n_bins=48), (32,) * 4),
         ("n64", "cqt", dict(filter_scale=0.25, n_bins=48), (64,) * 4),
         ("n128", "cqt", dict(filter_scale=0.5, window="hamming", sparsity=0.05), (128,) * 7),
         ("n256", "cqt", dict(), (256,) * 7),
         ("n512", "cqt", dict(bins_per_octave=24, n_bins=72), (512,) * 3),
         ("n1024", "cqt", dict(filter_scale=4, n_bins=48), (1024,) * 4),
         ("n2048", "cqt", dict(filter_scale=8, n_bins=48), (2048,) * 4),
         ("n4096", "cqt", dict(filter_scale=16, n_bins=36), (4096,) * 3),
         ("vqt-mixed", "vqt", dict(filter_scale=16, gamma=10.0, n_bins=84), (4096, 4096, 4096, 2048, 2048, 1024, 512)),
         ("n8192-two-launch", "cqt", dict(filter_scale=32, n_bins=36, hop_length=64), (8192,) * 3)]
WHOLE_IDS = [w[0] for w in WHOLE]
WHOLE_N = 16000   # samples (0.73 s at 22 050 Hz): longer than every frame length here, several groups of frames per octave, the oracle in a few seconds per case


def whole_signal(dtype):
    import golden_cases

    return golden_cases.make_signal("mix", WHOLE_N, 41, (2,), np.dtype(dtype).name)


def whole_plan(kw, dtype):
    """The octaves' frame lengths of a whole-transform case, by the library's own planner (host arithmetic only)."""
    from librosa_amd.core import constantq

    cplx = np.dtype(np.complex128 if np.dtype(dtype) == np.float64 else np.complex64)
    a = dict(sr=SR, hop_length=512, fmin=None, n_bins=84, gamma=0, bins_per_octave=12, filter_scale=1, norm=1, sparsity=0.01, window="hann", scale=True)
    a.update(kw)
    fmin = constantq._C1_HZ if a["fmin"] is None else a["fmin"]
    plan = constantq._plan(float(a["sr"]), int(a["hop_length"]), float(fmin), int(a["n_bins"]), "equal", None if a["gamma"] is None else float(a["gamma"]), int(a["bins_per_octave"]),
                           float(a["filter_scale"]), float(a["norm"]), float(a["sparsity"]), a["window"], bool(a["scale"]), cplx.str)
    return tuple(o["n_fft"] for o in plan["octaves"])


_ORACLE = {}


def whole_oracle(name, dtype):
    """cqt_oracle's transform of a whole case, computed once."""
    import cqt_oracle as CQ

    key = (name, np.dtype(dtype).str)
    if key not in _ORACLE:
        _, fn, kw, _ = WHOLE[WHOLE_IDS.index(name)]
        ref = getattr(CQ, fn)(whole_signal(dtype), sr=SR, res_type="polyphase", **kw)
        ref.setflags(write=False)
        _ORACLE[key] = ref
    return _ORACLE[key]
