"""oracle/rhythm_oracle.py pinned to the reference: every case of tests/golden/onset.npz, rhythm.npz and beat.npz with the bounds the host
simulators meet on the same fixtures, and the edge cases of tests/golden/rhythm_edges.npz.  Also the properties of the edge table that only
need the oracle: every beat case certified at the fixture's radius, and at least 0.9 of every tempo case's decisions clear of rounding."""
import json
import os

import numpy as np
import pytest

import beat_signals as BS
import rhythm_cases as RC
import rhythm_edges as E
import rhythm_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- onset.npz --------------------------------------------------------------------------------------------------------------------------------
def p75(x, axis):
    return np.percentile(x, 75, axis=axis)


ONSET_AGG = dict(E.AGGREGATES, p75=p75)
ONSET = np.load(os.path.join(HERE, "golden", "onset.npz"))
ONSET_CASES = json.loads(str(ONSET["cases"]))


def _power_to_db(S):
    """10 log10(max(1e-10, |S|)) floored 80 dB below the array's maximum, in S's dtype."""
    S = np.abs(S)
    db = (10.0 * np.log10(np.maximum(S.dtype.type(1e-10), S))).astype(S.dtype)
    return np.maximum(db, db.max() - S.dtype.type(80.0))


@pytest.mark.parametrize("name", sorted(ONSET_CASES))
def test_onset_oracle_matches_the_reference(name):
    case = ONSET_CASES[name]
    kw = dict(case["kwargs"])
    ref = None
    if case["mel"] is not None:
        S = ONSET[f"db_{case['mel']}"]
    elif "feature" in kw:
        S = _power_to_db(ONSET[f"feature_out_{name}"])
    else:
        S = np.atleast_2d(ONSET[case["input"]])
        ref = ONSET[kw["ref"]] if isinstance(kw.get("ref"), str) else None
    channels = kw.get("channels")
    if isinstance(channels, dict):
        channels = [slice(a, b) for a, b in channels["slices"]]
    center_pad = kw.get("n_fft", 2048) // (2 * kw.get("hop_length", 512)) if kw.get("center", True) else None
    got = O.onset_multi(S, lag=kw.get("lag", 1), max_size=kw.get("max_size", 1), ref=ref, channels=channels, aggregate=ONSET_AGG[case["aggregate"]], center_pad=center_pad,
                        detrend=kw.get("detrend", False))
    if case["fn"] == "strength":
        got = got[..., 0, :]
    want = ONSET[name]
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    if ok.any():
        scale = np.max(np.abs(want[ok]))
        err = np.max(np.abs(got[ok].astype(np.float64) - want[ok]))
        assert err <= (1e-12 if want.dtype == np.float64 and "f64" in name else 1e-5) * max(scale, 1e-30), f"{name}: {err:.3e} of {scale:.3e}"


# ---- rhythm.npz -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rhythm():
    return RC.load()


@pytest.mark.parametrize("name", RC.names("tempogram"))
def test_tempogram_oracle_matches_the_reference(rhythm, name):
    z, cases, inputs = rhythm
    call = RC.call_kwargs(cases[name]["kwargs"], inputs)
    got = O.tempogram(z[f"env_{name}"], win_length=call.get("win_length", 384), center=call.get("center", True), window=call.get("window", "hann"), norm=call.get("norm", np.inf))
    assert got.dtype == np.float64
    assert RC.col_err(RC.sampled(z, name, got), z[name]) <= 1e-13


@pytest.mark.parametrize("name", RC.names("tempo"))
def test_tempo_oracle_matches_the_reference(rhythm, name):
    z, cases, inputs = rhythm
    call = RC.call_kwargs(cases[name]["kwargs"], inputs)
    call.setdefault("aggregate", np.mean)
    env = z[f"env_{name}"]
    if cases[name]["input"].startswith("tg:"):
        got, margin = O.tempo(tg=O.tempogram(env), **call)
    else:
        got, margin = O.tempo(env, **call)
    W = len(z[f"bpms_{name}"])
    bpms, lp = O.tempo_tables(W, **{k: v for k, v in call.items() if k != "aggregate"})
    np.testing.assert_array_equal(bpms, z[f"bpms_{name}"])
    np.testing.assert_array_equal(lp, z[f"logprior_{name}"])
    want, ref_margin = z[name], z[f"margin_{name}"].reshape(z[name].shape)
    assert got.shape == want.shape
    ok = ref_margin >= 1e-9
    assert ok.mean() >= 0.9
    np.testing.assert_array_equal(got[ok], want[ok])
    fin = np.isfinite(ref_margin) & ok
    assert np.allclose(margin.reshape(want.shape)[fin], ref_margin[fin], rtol=1e-6, atol=1e-10)


# ---- beat.npz ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def beat():
    return BS.load()


def _dense(want, shape):
    if want.dtype == bool:
        return want
    dense = np.zeros(shape, bool)
    dense[want] = True
    return dense


@pytest.mark.parametrize("name", BS.names())
def test_beat_oracle_matches_the_reference(beat, name):
    z, cases, _, params = beat
    kw = BS.call_kwargs(cases[name]["kwargs"], z, name)
    env = z[f"env_{name}"]
    sr, hop = kw.get("sr", BS.SR), kw.get("hop_length", 512)
    if name.startswith("zero_"):
        assert not O.beat_track(env, bpm=120.0, frame_rate=sr / hop)[0].any() and not z[f"beats_{name}"].any()
        return
    bpm = kw["bpm"] if "bpm" in kw else z[f"tempo_{name}"]
    beats, ls, cum, _ = O.beat_track(env, bpm=bpm, frame_rate=float(sr) / hop, tightness=kw.get("tightness", 100), trim=kw.get("trim", True))
    for got, key in ((ls, "ls"), (cum, "cum")):
        want = z[f"{key}_{name}"]
        assert got.dtype == want.dtype
        scale = np.max(np.abs(want))
        assert (np.max(np.abs(got.astype(np.float64) - want)) / scale if scale > 0 else 0.0) <= params["radius"]
    want = z[f"beats_{name}"]
    if kw.get("units") == "samples":
        np.testing.assert_array_equal(np.flatnonzero(beats) * hop, want)
    elif kw.get("units") == "time":
        np.testing.assert_array_equal(np.flatnonzero(beats) * hop / float(sr), want)
    else:
        np.testing.assert_array_equal(beats, _dense(want, env.shape))


@pytest.mark.parametrize("row", BS.FULL_STORED)
def test_beat_oracle_matches_the_reference_full_rows(beat, row):
    z = beat[0]
    env = z[f"full_env_{row}"]
    beats = O.beat_track(env, bpm=z[f"full_tempo_{row}"], frame_rate=BS.SR / 512)[0]
    np.testing.assert_array_equal(np.flatnonzero(beats), z[f"full_beats_{row}"])


# ---- rhythm_edges.npz -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edges():
    return E.load()


def test_edge_fixture_is_small_and_made_from_these_inputs(edges):
    z, params = edges
    assert os.path.getsize(E.GOLDEN) < 1 << 20
    assert {"numpy", "scipy", "reference_version", "radius", "draws"} <= set(params) and params["radius"] == E.RADIUS and params["draws"] == E.DRAWS
    for name in E.GOLDEN_TG:
        assert float(z[f"sum_tg_{name}"]) == E.checksum(E.tg_envelope(E.TG_CASES[name])), name
    for name in E.GOLDEN_BEAT:
        assert float(z[f"sum_beat_{name}"]) == E.checksum(E.beat_inputs(E.BEAT_CASES[name])[0]), name
    for name in E.GOLDEN_ONSET:
        assert float(z[f"sum_onset_{name}"]) == E.checksum(E.onset_input(E.ONSET_CASES[name])), name


@pytest.mark.parametrize("name", E.GOLDEN_TG)
def test_edge_tempogram_oracle_matches_the_reference(edges, name):
    z, _ = edges
    case = E.TG_CASES[name]
    env = E.tg_envelope(case)
    got = O.tempogram(env, win_length=case["W"], center=case["center"], norm=E.NORMS[case["norm"]])
    assert RC.col_err(got[..., z[f"cols_tg_{name}"]], z[f"tg_{name}"]) <= 1e-13
    if E.SUM in case["modes"]:
        for key, agg in (("mean", np.mean), ("none", None)):
            bpm, _ = O.tempo(env, aggregate=agg, **E.tempo_kwargs(case))
            want, margin = z[f"tempo_{key}_{name}"], z[f"margin_{key}_{name}"]
            ok = margin >= 1e-9
            assert ok.mean() >= 0.9
            np.testing.assert_array_equal(bpm[ok], want[ok])


def _beat_call(case):
    return dict(frame_rate=E.FRAME_RATE, tightness=case["tightness"], trim=case["trim"])


@pytest.fixture(scope="module")
def beat_oracle():
    """The oracle's result of every beat case, computed once."""
    out = {}
    for name, case in E.BEAT_CASES.items():
        env, bpm = E.beat_inputs(case)
        out[name] = (env, bpm) + O.beat_track(env, bpm=bpm, **_beat_call(case))
    return out


@pytest.mark.parametrize("name", E.GOLDEN_BEAT)
def test_edge_beat_oracle_matches_the_reference(edges, beat_oracle, name):
    z, params = edges
    env, bpm, beats, ls, cum, _ = beat_oracle[name]
    live = env.reshape(-1, env.shape[-1]).any(axis=-1).reshape(env.shape[:-1])  # (the reference ran the live rows one by one)
    for got, key in ((ls, "ls"), (cum, "cum")):
        want = z[f"{key}_beat_{name}"]
        assert got.dtype == want.dtype
        g, w = got[live].astype(np.float64), want[live]
        assert np.max(np.abs(g - w)) <= params["radius"] * np.max(np.abs(w))
    np.testing.assert_array_equal(beats, z[f"beats_beat_{name}"])
    assert beats[live].any(axis=-1).all() and not beats[~live].any()


@pytest.mark.parametrize("name", list(E.BEAT_CASES))
def test_every_beat_case_is_certified(beat_oracle, name):
    case = E.BEAT_CASES[name]
    env, bpm, beats = beat_oracle[name][:3]
    if env.ndim == 1:
        assert O.certify(env, dict(bpm=bpm, **_beat_call(case)), beats, E.RADIUS, E.DRAWS)
    else:  # row by row: the noise radius follows each row's own maximum, and the all-zero row stays all zero
        for r in range(len(env)):
            assert O.certify(env[r], dict(bpm=bpm[r], **_beat_call(case)), beats[r], E.RADIUS, E.DRAWS), r


def test_half_even_tempi_are_exact():
    for f in (20.5, 21.5, 2.0, 1024.0, 1025.0):
        assert E.FRAME_RATE * 60.0 / E.bpm_of(f) == f
    assert np.round(20.5) == 20 and np.round(21.5) == 22


@pytest.mark.parametrize("name", [n for n, c in E.TG_CASES.items() if E.SUM in c["modes"]])
def test_tempo_cases_have_margin(name):
    case = E.TG_CASES[name]
    env = E.tg_envelope(case)
    for agg in (np.mean, None):
        _, margin = O.tempo(env, aggregate=agg, **E.tempo_kwargs(case))
        assert np.mean(margin >= 1e-9) >= 0.9


@pytest.mark.parametrize("name", E.GOLDEN_ONSET)
def test_edge_onset_oracle_matches_the_reference(edges, name):
    z, _ = edges
    case = E.ONSET_CASES[name]
    got = O.onset_multi(E.onset_input(case), **E.onset_kwargs(case))
    want = z[f"onset_{name}"]
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    if ok.any():
        scale = max(float(np.max(np.abs(want[ok]))), 1e-30)
        assert np.max(np.abs(got[ok].astype(np.float64) - want[ok])) <= (1e-12 if case["dtype"] == "float64" else 1e-5) * scale


def test_refused_window_lengths_are_where_the_layout_says():
    w, s = E.first_refused(E.WRITE), E.first_refused(E.SUM)
    assert 10000 < w < 10600 and 6600 < s < 7000
    assert E.lds_total(w - 1, E.WRITE, False) <= E.LDS_MAX < E.lds_total(w, E.WRITE, False)
    assert E.lds_total(s - 1, E.SUM, False) <= E.LDS_MAX < E.lds_total(s, E.SUM, False)
