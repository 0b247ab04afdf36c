"""The edge-case table of tests/rhythm_edges.py through the host simulators of the kernel bodies (tests/hostsim/rhythmsim.cpp, beatsim.cpp,
onsetsim.cpp) against oracle/rhythm_oracle.py: every transform size of the tempogram kernel, the direct kernel, the tiled and untiled
WRITE epilogue, the beat tracker's ring wrap and its 2048 boundary, the median kernel down to one frame per workgroup."""
import numpy as np
import pytest

import rhythm_cases as RC
import rhythm_edges as E
import rhythm_oracle as O
from librosa_amd import onset as ON
from librosa_amd.feature import rhythm as R
from test_beat_host import sim_exec as beat_sim
from test_onset_host import sim_exec as onset_sim
from test_rhythm_host import sim_exec as rhythm_sim


# ---- tempogram / tempo ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.TG_CASES))
def test_simulated_tempogram_kernels_match_the_oracle(name):
    case = E.TG_CASES[name]
    env, W = E.tg_envelope(case), case["W"]
    window = O._window("hann", W)
    want = O.tempogram(env, win_length=W, center=case["center"], norm=E.NORMS[case["norm"]])
    got, bad = rhythm_sim(env, W, case["center"], window, R._norm_code(E.NORMS[case["norm"]]), R._WRITE)
    assert not bad and got.shape == want.shape and not np.isnan(got).any()
    err = RC.col_err(got, want)
    print(f"{name}: N = {E.transform_length(W)}, error {err:.3g} of the column maximum")
    assert err <= 1e-13
    if E.SUM not in case["modes"]:
        return
    kw = E.tempo_kwargs(case)
    bpms, lp = R._tables(W, kw["hop_length"], kw["sr"], 120, 1.0, 320.0, None)
    for mode, agg in ((R._SUM, np.mean), (R._ARGMAX, None)):
        want, margin = O.tempo(env, aggregate=agg, **kw)
        got, bad = rhythm_sim(env, W, True, window, R._NORM_INF, mode, lp, bpms)
        assert not bad
        got = got.reshape(want.shape)
        ok = margin >= 1e-9
        assert ok.mean() >= 0.9
        np.testing.assert_array_equal(got[ok], want[ok])


# ---- beat tracker -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.BEAT_CASES))
def test_simulated_tracker_matches_the_oracle(name):
    case = E.BEAT_CASES[name]
    env, bpm = E.beat_inputs(case)
    want, ls_w, cum_w, _ = O.beat_track(env, bpm=bpm, frame_rate=E.FRAME_RATE, tightness=case["tightness"], trim=case["trim"])
    beats, ls, cum, _, alive = beat_sim(env, bpm, E.FRAME_RATE, case["tightness"], case["trim"])
    assert alive and ls.dtype == ls_w.dtype
    live = env.reshape(-1, env.shape[-1]).any(axis=-1).reshape(env.shape[:-1])
    for got, ref, key in ((ls, ls_w, "local score"), (cum, cum_w, "cumulative score")):
        err = np.max(np.abs(got[live].astype(np.float64) - ref[live])) / np.max(np.abs(ref[live]))
        print(f"{name}: {key} error {err:.3g} of the maximum")
        assert err <= E.RADIUS
    np.testing.assert_array_equal(beats, want)
    assert want[live].any(axis=-1).all() and not beats[~live].any()


# ---- onset strength ---------------------------------------------------------------------------------------------------------------------------
def _onset_sim(case, S, detrend):
    kw = E.onset_kwargs(case)
    agg = kw["aggregate"]
    code = ON._NONE if agg is False else next(c for f, c in ON._DEVICE_AGGREGATES if agg is f)
    job = dict(lag=case["lag"], max_size=case["max_size"], code=code, aggregate=agg, channels=kw["channels"], pad_width=case["lag"] + 2, center=True, detrend=detrend)
    S3 = S.reshape((-1,) + S.shape[-2:])
    n_out = ON._out_frames(max(S3.shape[-1] - case["lag"], 0), job, S3.shape[-1])
    out = onset_sim(S3, None, job, code, job["pad_width"], n_out)
    return out.reshape(S.shape[:-2] + out.shape[1:])


@pytest.mark.parametrize("name", list(E.ONSET_CASES))
def test_simulated_onset_kernels_match_the_oracle(name):
    case = E.ONSET_CASES[name]
    S = E.onset_input(case)
    E.check_onset(case, _onset_sim(case, S, case["detrend"]), S, lambda: _onset_sim(case, S, False))


def test_median_table_reaches_every_workgroup_width():
    """64, 32, 16, 8, 4, 2 and 1 frames per workgroup (lra_onset.h: onset_median_frames), the last at exactly 160 KiB."""
    def frames(bands, elem):
        fb = 64
        while fb > 1 and bands * fb * elem > 64 * 1024:
            fb //= 2
        return fb if bands * fb * elem <= 160 * 1024 else 0

    f32 = {frames(c["bands"], 4) for n, c in E.ONSET_CASES.items() if n.startswith("median_f32_")}
    assert f32 == {64, 32, 16, 8, 4, 2, 1}
    assert {frames(c["bands"], 8) for n, c in E.ONSET_CASES.items() if n.startswith("median_f64_")} == {64, 32, 1}
    assert frames(40960, 4) == 1 and 40960 * 4 == 160 * 1024 and frames(E.ONSET_REFUSED_BANDS, 4) == 0
