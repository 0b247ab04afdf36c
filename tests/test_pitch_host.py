"""piptrack / pitch_tuning / estimate_tuning without a GPU: every argument error before any device work, the host converters, the NumPy
model against tests/golden/pitch.npz, and every kernel body of librosa_amd/csrc/lra_pitch.h run on the host (tests/hostsim/pitchsim.cpp)
on every fixture case under the bounds of tests/pitch_cases.py: both layouts of the dense tracker, the emitting variant against the dense
one, the radix select against np.median, and the histogram against np.histogram."""
import ctypes
import json
import warnings

import numpy as np
import pytest

import hostsim_util
import librosa_amd as L
import pitch_cases as PC
from librosa_amd.core import pitch as pitch_mod

REF_MAX, REF_ROW, REF_SCALAR = 0, 1, 2


@pytest.fixture(scope="module")
def golden():
    z = np.load(PC.GOLDEN)
    return z, json.loads(bytes(z["meta"]).decode())


# ---- arguments, converters, exports -------------------------------------------------------------------------------------------------------
def test_the_names_are_exported():
    for name in ("piptrack", "pitch_tuning", "estimate_tuning", "hz_to_octs", "octs_to_hz"):
        assert getattr(L, name) is getattr(L.core, name)
    assert L.piptrack is pitch_mod.piptrack


def test_every_argument_error_comes_before_device_work(golden):
    _, meta = golden
    y = np.zeros(4096, np.float32)
    S = np.ones((33, 4), np.float32)
    assert meta["errors"]["no_input"] == meta["errors"]["n_fft_none"] == meta["errors"]["tuning_no_input"] == "ParameterError"
    for call in (lambda: L.piptrack(sr=PC.SR), lambda: L.piptrack(y=y, n_fft=None), lambda: L.estimate_tuning(sr=PC.SR), lambda: L.estimate_tuning(y=y, n_fft=None),
                 lambda: L.piptrack(S=S, sr=0), lambda: L.piptrack(S=S, threshold="x"), lambda: L.piptrack(S=S, ref="max"), lambda: L.piptrack(S=S, fmin=None),
                 lambda: L.piptrack(S=np.ones(33, np.float32)), lambda: L.piptrack(S=np.ones((33, 4), np.int32)), lambda: L.estimate_tuning(S=S, resolution=0),
                 lambda: L.estimate_tuning(S=S, resolution=-0.1), lambda: L.estimate_tuning(S=S, bins_per_octave=0), lambda: L.pitch_tuning([440.0], resolution=0),
                 lambda: L.pitch_tuning(np.array([1 + 2j]))):
        with pytest.raises(L.ParameterError):
            call()
    assert meta["errors"]["tuning_bad_kwarg"] == "TypeError"
    with pytest.raises(TypeError, match="nonsense"):
        L.estimate_tuning(y=y, nonsense=1)


def test_fewer_than_two_bins_is_a_documented_difference(golden):
    _, meta = golden
    assert meta["errors"]["one_bin"] == "ZeroDivisionError"  # the reference fails incidentally
    for call in (lambda: L.piptrack(S=np.ones((1, 4), np.float32)), lambda: L.estimate_tuning(S=np.ones((2, 1, 4), np.float64))):
        with pytest.raises(L.ParameterError, match="at least 2 frequency bins"):
            call()


def test_empty_sets_warn_and_return_zero_without_a_device(golden):
    _, meta = golden
    for name in ("empty",):
        assert meta["pitch_tuning"][name] == dict(value=0.0, warned=["Trying to estimate tuning from empty frequency set."], freqs=PC.digest(PC.PITCH_TUNING[name]["freqs"]))
        with pytest.warns(UserWarning, match="Trying to estimate tuning from empty frequency set."):
            assert L.pitch_tuning(PC.PITCH_TUNING[name]["freqs"]) == 0.0
    with pytest.warns(UserWarning, match="empty frequency set"):
        assert L.estimate_tuning(S=np.ones((33, 0), np.float32)) == 0.0


def test_host_converters():
    assert L.hz_to_octs(440.0) == 4.0 and isinstance(L.hz_to_octs(440.0), np.float64)
    assert np.allclose(L.hz_to_octs([32, 64, 128, 256]), [0.219, 1.219, 2.219, 3.219], atol=5e-4)
    assert L.octs_to_hz(1) == 55.0 and np.array_equal(L.octs_to_hz([-2, -1, 0, 1, 2]), [6.875, 13.75, 27.5, 55.0, 110.0])
    f = np.array([27.5, 100.0, 4186.0])
    assert np.allclose(L.octs_to_hz(L.hz_to_octs(f, tuning=0.3, bins_per_octave=24), tuning=0.3, bins_per_octave=24), f, rtol=1e-14)
    assert L.hz_to_octs(440.0 * 2 ** (0.5 / 12), tuning=0.5) == pytest.approx(4.0, abs=1e-14)


def test_the_bin_range_is_the_reference_mask():
    for sr, n_fft, fmin, fmax in ((22050, 2048, 150.0, 4000.0), (6400, 64, 300.0, 1500.0), (22050, 65, 0.0, 22050.0), (22050, 2, 0.0, 1e9), (8000, 512, -5.0, 3999.9), (8000, 512, 5000.0, 6000.0)):
        freqs = np.fft.rfftfreq(n_fft, 1.0 / sr)
        mask = (max(fmin, 0) <= freqs) & (freqs < min(fmax, sr / 2))
        lo, hi = pitch_mod._bin_range(sr, n_fft, fmin, fmax)
        assert np.array_equal(mask, (np.arange(freqs.size) >= lo) & (np.arange(freqs.size) < hi))
    assert pitch_mod._bin_range(6400, 64, 300.0, 1500.0) == (3, 15)


# ---- the model against the golden ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.PIP))
def test_model_against_the_reference(golden, name):
    z, meta = golden
    S = PC.pip_input(name)
    assert PC.digest(S) == meta["inputs"][name]
    with np.errstate(all="ignore"):
        mp, mm = PC.model_piptrack(S, **PC.pip_kwargs(name))
    for got, want in ((mp, z["pitches_" + name]), (mm, z["mags_" + name])):
        assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got != 0, want != 0)
        assert PC.ulp_distance(got, want) <= 1
    # the float64 model: the same peaks wherever no comparison is within rounding (asserted for every case: none is)
    S64 = S.astype(np.complex128 if np.iscomplexobj(S) else np.float64)
    with np.errstate(all="ignore"):
        p64, m64 = PC.model_piptrack(S64, **PC.pip_kwargs(name))
    if PC.PIP[name]["kind"] != "complex" and "ref" not in PC.PIP[name]["kw"] and PC.PIP[name]["kw"].get("threshold", 0.1) not in (1.0,):
        assert np.array_equal(p64 != 0, mp != 0)
        assert np.allclose(p64, mp, rtol=1e-4 if S.dtype == np.float32 else 1e-12, atol=0)


@pytest.mark.parametrize("name", list(PC.TUNING))
def test_tuning_cases_are_certified(golden, name):
    _, meta = golden
    y = PC.tuning_signal(name)
    S = PC.host_magnitudes(y)
    assert PC.digest(y) == meta["tuning"][name]["y"] and PC.digest(S) == meta["tuning"][name]["S"]
    kw = PC.tuning_kwargs(name)
    assert PC.certify_tuning(S, kw["resolution"], kw["bins_per_octave"], sr=kw["sr"], n_fft=kw["n_fft"]) == []
    got, counts = PC.model_estimate_tuning(S.astype(np.float64), kw["resolution"], kw["bins_per_octave"], sr=kw["sr"], n_fft=kw["n_fft"])
    assert got == meta["tuning"][name]["from_S"] == meta["tuning"][name]["from_y"]
    assert np.sort(counts)[-1] - np.sort(counts)[-2] == meta["tuning"][name]["lead"] >= 3
    assert {m["peaks"] % 2 for k, m in meta["tuning"].items() if k != "silence"} == {0, 1}


@pytest.mark.parametrize("name", list(PC.PITCH_TUNING))
def test_pitch_tuning_model(golden, name):
    _, meta = golden
    c = PC.PITCH_TUNING[name]
    assert PC.digest(c["freqs"]) == meta["pitch_tuning"][name]["freqs"]
    assert PC.model_pitch_tuning(c["freqs"], **c["kw"])[0] == meta["pitch_tuning"][name]["value"]
    assert meta["pitch_tuning"]["cqt_quarter"]["value"] == 0.25


# ---- the kernel bodies on the host -----------------------------------------------------------------------------------------------------------
_sim = None


def sim_lib():
    global _sim
    if _sim is None:
        _sim = hostsim_util.sim_lib("pitchsim", pthread=False)
        c = ctypes
        front = [c.c_void_p] + [c.c_longlong] * 6 + [c.c_int, c.c_longlong, c.c_longlong, c.c_int, c.c_double, c.c_void_p, c.c_double, c.c_double, c.c_longlong]
        _sim.pitchsim_piptrack.argtypes = front + [c.c_void_p, c.c_void_p] + [c.c_longlong] * 3
        _sim.pitchsim_tuning.argtypes = front + [c.c_void_p, c.c_longlong, c.c_double, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_void_p, c.c_void_p]
        _sim.pitchsim_median.argtypes = [c.c_void_p, c.c_void_p, c.c_longlong, c.c_int, c.c_int, c.c_int, c.c_void_p, c.POINTER(c.c_ulonglong)]
        _sim.pitchsim_pitch_tuning.argtypes = [c.c_void_p, c.c_longlong, c.c_int, c.c_void_p, c.c_longlong, c.c_double, c.c_void_p]
        _sim.pitchsim_hist_bin.argtypes = [c.c_void_p, c.c_int, c.c_double]
    return _sim


def test_the_cases_sit_on_the_kernels_geometry():
    sim = sim_lib()
    assert sim.pitchsim_const(0) == PC.STAGE_TILE
    assert max(c["n_bins"] for c in PC.PIP.values()) > PC.STAGE_TILE + 1                                       # a row that crosses the staging-tile seam
    assert max(c["n_frames"] for c in PC.PIP.values() if c["layout"] == "fm") > sim.pitchsim_const(1)          # more than one workgroup, frame-major
    assert max(c["n_frames"] for c in PC.PIP.values() if c["layout"] == "bm") > sim.pitchsim_const(2)          # and bin-major
    assert max(PC.tuning_edges(c["kw"].get("resolution", 0.01)).size - 1 for c in PC.PITCH_TUNING.values()) > sim.pitchsim_const(4)  # the global histogram
    assert max(c["freqs"].size for c in PC.PITCH_TUNING.values()) > 2 * sim.pitchsim_const(5)


def _front(S, kw, form, pad=3):
    """The arguments lra_piptrack_exec / lra_tuning_exec share, as core/pitch.py sets them up, on the real magnitudes of ``S``.
    form "rows": [b][t][pitch] with ``pad`` poisoned elements behind every row; "cols": [b][f][t]."""
    S = np.abs(S) if np.iscomplexobj(S) else S
    real = S.dtype
    lead, (n_bins, n_frames) = S.shape[:-2], S.shape[-2:]
    batch = int(np.prod(lead)) if lead else 1
    n_fft = kw.get("n_fft", 2048)
    if n_fft // 2 + 1 != n_bins:
        n_fft = 2 * (n_bins - 1)
    lo, hi = pitch_mod._bin_range(kw["sr"], n_fft, kw.get("fmin", 150.0), kw.get("fmax", 4000.0))
    if form == "rows":
        pitch = n_bins + pad
        A = np.full((batch, n_frames, pitch), np.nan, real)  # (the padding behind the rows must never be read)
        A[..., :n_bins] = np.swapaxes(S, -1, -2).reshape(batch, n_frames, n_bins)
        strides = (n_frames * pitch, 1, pitch)
    else:
        A = np.ascontiguousarray(S).reshape(batch, n_bins, n_frames)
        strides = (n_bins * n_frames, n_frames, 1)
    ref, threshold = kw.get("ref"), kw.get("threshold", 0.1)
    row = None
    if ref is None or ref is np.max:
        mode, scalar = REF_MAX, 0.0
    elif callable(ref):
        mode, scalar, row = REF_ROW, 0.0, pitch_mod._host_ref_row(S, ref, threshold, tuple(lead), n_frames)
    else:
        mode, scalar = REF_SCALAR, float(np.abs(ref))
    args = [A.ctypes.data, batch, n_bins, n_frames, *strides, int(real == np.float64), lo, hi, mode, float(threshold), None if row is None else row.ctypes.data, scalar, float(kw["sr"]), n_fft]
    return args, (A, row), dict(batch=batch, n_bins=n_bins, n_frames=n_frames, real=real, lead=tuple(lead), lo=lo, hi=hi)


def sim_piptrack(S, kw, form):
    args, keep, d = _front(S, kw, form)
    batch, n_bins, n_frames = d["batch"], d["n_bins"], d["n_frames"]
    if form == "rows":
        out = np.full((2, batch, n_frames, n_bins), np.nan, d["real"])
        ostr = (n_frames * n_bins, 1, n_bins)
    else:
        out = np.full((2, batch, n_bins, n_frames), np.nan, d["real"])
        ostr = (n_bins * n_frames, n_frames, 1)
    assert sim_lib().pitchsim_piptrack(*args, out[0].ctypes.data, out[1].ctypes.data, *ostr) == 0
    res = np.swapaxes(out, -1, -2) if form == "rows" else out
    res = res.reshape((2,) + d["lead"] + (n_bins, n_frames))
    return res[0], res[1]


def sim_tuning(S, kw, form, resolution=0.05, bins_per_octave=12):
    """-> (counts row [n_hist + 2], thr, emitted pitches [frames][cap], mags, per-frame counts)."""
    args, keep, d = _front(S, kw, form)
    frames = d["batch"] * d["n_frames"]
    cap = (max(d["hi"] - d["lo"], 1) + 1) // 2
    pk_p, pk_m = np.full((frames, cap), np.nan, d["real"]), np.full((frames, cap), np.nan, d["real"])
    pk_n = np.full(frames, -1, np.int32)
    edges = PC.tuning_edges(resolution)
    out = np.zeros(edges.size + 1, np.uint64)
    thr = np.zeros(1, d["real"])
    assert sim_lib().pitchsim_tuning(*args, edges.ctypes.data, edges.size - 1, float(bins_per_octave), pk_p.ctypes.data, pk_m.ctypes.data, pk_n.ctypes.data, cap, out.ctypes.data,
                                     thr.ctypes.data) == 0
    return out.astype(np.int64), thr[0], pk_p, pk_m, pk_n


@pytest.mark.parametrize("name", list(PC.PIP))
def test_sim_piptrack_every_case_both_forms(golden, name):
    z, _ = golden
    S, kw = PC.pip_input(name), PC.pip_kwargs(name)
    for form in ("rows", "cols"):
        pitches, mags = sim_piptrack(S, kw, form)
        for got, want in ((pitches, z["pitches_" + name]), (mags, z["mags_" + name])):
            assert got.shape == want.shape and got.dtype == want.dtype
            assert not np.isnan(got).any(), "every element is written"
            assert np.array_equal(got != 0, want != 0), (form, "peak positions")
            assert PC.ulp_distance(got, want) <= PC.ULPS, form


@pytest.mark.parametrize("name", list(PC.PIP))
def test_sim_emitting_variant_median_and_counts(name):
    """The emitting variant gives the dense one's peaks in bin order, the radix select np.median of their magnitudes, and the histogram takes
    exactly the peaks at or above it."""
    S, kw = PC.pip_input(name), PC.pip_kwargs(name)
    for form in ("rows", "cols"):
        pitches, mags = sim_piptrack(S, kw, form)
        row, thr, pk_p, pk_m, pk_n = sim_tuning(S, kw, form)
        P = np.moveaxis(pitches, -2, -1).reshape(-1, pitches.shape[-2])  # [frame][bin]
        M = np.moveaxis(mags, -2, -1).reshape(-1, pitches.shape[-2])
        all_m = []
        for i in range(P.shape[0]):
            hit = np.flatnonzero(P[i] > 0)
            assert pk_n[i] == hit.size
            assert np.array_equal(pk_p[i, : hit.size], P[i, hit]) and np.array_equal(pk_m[i, : hit.size], M[i, hit])
            all_m.append(M[i, hit])
        all_m = np.concatenate(all_m) if all_m else np.zeros(0, S.dtype)
        assert row[-1] == all_m.size
        want_thr = np.median(all_m) if all_m.size else 0.0
        assert thr == want_thr and thr.dtype == all_m.dtype
        assert row[-2] == (all_m >= want_thr).sum() == row[:-2].sum()


@pytest.mark.parametrize("name", list(PC.TUNING))
def test_sim_estimate_tuning_certified_cases(golden, name):
    _, meta = golden
    kw = PC.tuning_kwargs(name)
    S = PC.host_magnitudes(PC.tuning_signal(name))
    want, counts = PC.model_estimate_tuning(S.astype(np.float64), kw["resolution"], kw["bins_per_octave"], sr=kw["sr"], n_fft=kw["n_fft"])
    edges = PC.tuning_edges(kw["resolution"])
    rows = []
    for form in ("rows", "cols"):
        row, thr, *_ = sim_tuning(S, dict(sr=kw["sr"], n_fft=kw["n_fft"]), form, kw["resolution"], kw["bins_per_octave"])
        assert np.array_equal(row[:-2], counts), form
        assert row[-1] == meta["tuning"][name]["peaks"]
        assert float(edges[np.argmax(row[:-2])]) == want == meta["tuning"][name]["from_S"]
        rows.append(row)
    assert np.array_equal(rows[0], rows[1])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sim_radix_select_is_np_median(dtype):
    rng = np.random.default_rng(5)
    sim = sim_lib()
    for n_seg, cap, grid in ((1, 1, 0), (1, 2, 0), (3, 5, 0), (40, 7, 3), (257, 9, 0), (64, 33, 2)):
        for flavour in ("normal", "ties", "signed", "tiny"):
            mag = rng.standard_normal((n_seg, cap))
            if flavour == "normal":
                mag = np.abs(mag)
            elif flavour == "ties":
                mag = np.round(np.abs(mag) * 3) / 3
            elif flavour == "tiny":
                mag = np.abs(mag) * 1e-40  # denormal in float32
            mag = mag.astype(dtype)
            count = rng.integers(0, cap + 1, n_seg).astype(np.int32)
            if flavour == "normal":
                count[:] = cap
            vals = np.concatenate([mag[i, : count[i]] for i in range(n_seg)])
            thr, total = np.zeros(1, dtype), ctypes.c_ulonglong(0)
            assert sim.pitchsim_median(mag.ctypes.data, count.ctypes.data, n_seg, cap, int(dtype == np.float64), grid, thr.ctypes.data, ctypes.byref(total)) == 0
            assert total.value == vals.size
            want = np.median(vals) if vals.size else dtype(0)
            assert thr[0] == want, (n_seg, cap, flavour, vals.size)


@pytest.mark.parametrize("name", list(PC.PITCH_TUNING))
def test_sim_pitch_tuning(golden, name):
    _, meta = golden
    c = PC.PITCH_TUNING[name]
    f = np.ascontiguousarray(c["freqs"])
    res, bpo = c["kw"].get("resolution", 0.01), c["kw"].get("bins_per_octave", 12)
    edges = PC.tuning_edges(res)
    out = np.zeros(edges.size + 1, np.uint64)
    assert sim_lib().pitchsim_pitch_tuning(f.ctypes.data, f.size, int(f.dtype == np.float64), edges.ctypes.data, edges.size - 1, float(bpo), out.ctypes.data) == 0
    assert out[-2] == (f > 0).sum() == out[:-2].sum()
    if out[-2]:
        assert float(edges[np.argmax(out[:-2])]) == meta["pitch_tuning"][name]["value"]
    if PC.pitch_tuning_margin(name) > (1e-4 if f.dtype == np.float32 else 1e-9) or name.startswith("fold"):
        assert np.array_equal(out[:-2].astype(np.int64), PC.model_pitch_tuning(f, res, bpo)[1])


def test_sim_histogram_bin_search_is_np_histogram():
    sim = sim_lib()
    rng = np.random.default_rng(9)
    for n in (1, 2, 10, 100, 5000):
        edges = np.linspace(-0.5, 0.5, n + 1)
        x = np.concatenate([edges, np.nextafter(edges, 1), np.nextafter(edges, -1), rng.random(200) - 0.5, [np.nan, 0.75, -0.75]])
        for v in x:
            got = sim.pitchsim_hist_bin(edges.ctypes.data, n, float(v))
            want = np.flatnonzero(np.histogram([v], edges)[0]) if np.isfinite(v) else np.zeros(0)
            assert got == (int(want[0]) if want.size else -1), (n, v)
    assert sim.pitchsim_hist_bin(edges.ctypes.data, n, 0.5) == n - 1  # the closed last bin
