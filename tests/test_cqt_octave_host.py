"""Every instance of the fused constant-Q octave kernel (csrc/lra_mixed.h: cqt_octave_body, eight frame lengths x two precisions) on the host simulator, against the
plain float64 reference of tests/cqt_cases.py at its per-row bar; the merged launch (mixed_cqt_multi_kernel) against the single launches, bit for bit; and the
assertions that keep the shared cases covering what they are for (the library's size list, each instance's frames per workgroup, the plans of the whole-transform
cases).  The device runs the same cases in tests/test_cqt_octave_gpu.py.
"""
import numpy as np
import pytest

import cqt_cases as C
import hostsim_util as H


def sim_octave(inst, run, c, y=None):
    """One octave launch through the simulator into a result that arrives full of NaN."""
    n_fft, dtype = inst
    y = c["y"] if y is None else y
    cplx = np.complex128 if np.dtype(dtype) == np.float64 else np.complex64
    out = np.full((y.shape[0], run["n_frames"], run["n_total"]), np.nan + 1j * np.nan, dtype=cplx)
    sl = c["sqrt_len"]
    H.cqt_octave(y.ctypes.data, y.shape[0], y.shape[1], y.shape[1], n_fft, run["hop"], run["pad_mode"], c["row_ptr"].ctypes.data, c["col"].ctypes.data, c["val"].ctypes.data,
                 sl.ctypes.data if sl is not None else None, out.ctypes.data, run["n_frames"], run["n_total"], run["bin0"], run["row0"], run["n_rows"], dtype)
    return out


def test_size_list_is_the_librarys():
    """The list the cases read from csrc/lra_mixed_sizes.h is the one the simulator was compiled with, every size is dispatched, and exactly one instance needs more
    than 64 KiB of dynamic LDS: float64 at the largest frame length, 98 336 bytes, which the simulated LDS holds."""
    assert C.SIZES == H.cqt_sizes()
    assert all(H.cqt_octave_supported(s) for s in C.SIZES) and not any(H.cqt_octave_supported(s) for s in (16, 48, 2 * max(C.SIZES)))
    big = [(n_fft, np.dtype(dt).name, H.cqt_lds_bytes(n_fft, dt)) for n_fft, dt in C.INSTANCES if H.cqt_lds_bytes(n_fft, dt) > 65536]
    assert big == [(4096, "float64", 98336)]


@pytest.mark.parametrize("inst", C.INSTANCES, ids=C.instance_id)
def test_family_covers_the_group_geometry(inst):
    """With the instance's own frames per workgroup: more frames than a group, a partial last group, at least two whole groups where F >= 5."""
    F = H.cqt_frames_per_group(*inst)
    assert 1 <= F <= 8
    C.check_family(inst, C.family(inst), F)


def test_frames_per_group_values():
    """Every value the budget gives is exercised: 8 and the reduced counts down to 1, in both types."""
    got = {np.dtype(dt).name: [H.cqt_frames_per_group(s, dt) for s in C.SIZES] for dt in C.DTYPES}
    assert all({1, 2, 5, 8} <= set(v) for v in got.values()), got


@pytest.mark.parametrize("inst", C.INSTANCES, ids=C.instance_id)
def test_octave_instance_through_simulator(inst):
    worst = 0.0
    for run in C.family(inst):
        c = C.build(inst, run)
        got = sim_octave(inst, run, c)
        ratio, msg = C.compare(got, c, run)
        print(msg)
        worst = max(worst, ratio / c["bar"])
        assert ratio <= c["bar"], msg
        bin0, n_rows = run["bin0"], run["n_rows"]
        assert np.isnan(got[:, :, :bin0]).all() and np.isnan(got[:, :, bin0 + n_rows :]).all(), (run["name"], "stored outside the octave's columns")
        if run["row0"] == 0:
            assert np.all(got[:, :, bin0] == 0), (run["name"], "the row without entries")
    print(f"{C.instance_id(inst)}: worst ratio / bar {worst:.3f}")


def _merged_case(n_fft, dtype, n_rows_list):
    """Octaves of one frame length and frame count that differ in signal, hop and rows: (octave dicts, arrays kept alive, n_frames, n_total, sqrt_len)."""
    rng = np.random.default_rng(n_fft + len(n_rows_list))
    row_ptr, col, val, sqrt_all = C.rows(n_fft, dtype)
    n_frames, batch = 11, 2
    octs, keep, top = [], [row_ptr, col, val], sum(n_rows_list) + 2
    n_total = top + 1
    for i, n_rows in enumerate(n_rows_list):
        hop = (3, 4, 7, 2)[i % 4] * max(1, n_fft // 32)
        n = hop * (n_frames - 1) + (5, 0, 3, 1)[i % 4]
        y = rng.standard_normal((batch, n)).astype(dtype)
        keep.append(y)
        top -= n_rows
        octs.append(dict(y=y.ctypes.data, n=n, y_stride=n, hop=hop, bin0=top, row0=(2, 0, 5, 1)[i % 4], n_rows=n_rows, row_ptr=row_ptr.ctypes.data, col=col.ctypes.data, val=val.ctypes.data))
    sqrt_len = np.sqrt(rng.random(n_total) * 50 + 1)
    return octs, keep, batch, n_frames, n_total, sqrt_len


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("n_fft", C.SIZES)
@pytest.mark.parametrize("n_rows_list", [(7, 10, 4), (6, 0, 5)], ids=["three", "one-empty"])
def test_merged_launch_equals_single_launches(n_fft, dtype, n_rows_list):
    """mixed_cqt_multi_kernel over several octaves == mixed_cqt_kernel once per octave, bit for bit, columns of no octave untouched; an octave without rows takes no
    blocks (lra_api.hip: cqt_octaves_merged)."""
    octs, keep, batch, n_frames, n_total, sqrt_len = _merged_case(n_fft, dtype, n_rows_list)
    cplx = np.complex128 if np.dtype(dtype) == np.float64 else np.complex64
    scaled = 0 not in n_rows_list   # (the scaling table, read from each octave's bin0 on, in one list; unscaled in the other)
    sl = sqrt_len.ctypes.data if scaled else None
    merged = np.full((batch, n_frames, n_total), np.nan + 1j * np.nan, dtype=cplx)
    H.cqt_octaves_merged(octs, batch, n_fft, "reflect", sl, merged.ctypes.data, n_frames, n_total, dtype)
    single = np.full_like(merged, np.nan + 1j * np.nan)
    for o in octs:
        if o["n_rows"]:
            H.cqt_octave(o["y"], batch, o["n"], o["y_stride"], n_fft, o["hop"], "reflect", o["row_ptr"], o["col"], o["val"], sl + 8 * o["bin0"] if scaled else None, single.ctypes.data, n_frames,
                         n_total, o["bin0"], o["row0"], o["n_rows"], dtype)
    assert np.array_equal(merged, single, equal_nan=True)
    written = np.zeros(n_total, bool)
    for o in octs:
        written[o["bin0"] : o["bin0"] + o["n_rows"]] = True
    assert np.isfinite(merged[:, :, written]).all() and np.isnan(merged[:, :, ~written]).all() and (~written).sum() >= 3


def test_whole_cases_reach_every_instance():
    """The cqt / vqt calls of cqt_cases.WHOLE plan (constantq._plan) the frame lengths written beside them: together every size of the list in both types, one case
    beyond the list (the two-launch route), and one of seven octaves that mixes frame lengths (the early merged pair, then one merged launch per run of equal lengths)."""
    for dt in C.DTYPES:
        reached = set()
        for name, fn, kw, want in C.WHOLE:
            plan = C.whole_plan(kw, dt)
            assert plan == want, (name, plan)
            reached |= set(plan)
        assert reached >= set(C.SIZES)
        assert any(all(not H.cqt_octave_supported(n) for n in w[3]) for w in C.WHOLE)
        assert any(len(w[3]) == 7 and len(set(w[3])) > 1 and w[1] == "vqt" for w in C.WHOLE)
