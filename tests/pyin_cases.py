"""The cases of the pyin tests, a NumPy model of ``__pyin_helper`` written from the reference line by line, and the rules of the checks.

TEST INFRASTRUCTURE ONLY.  ``scripts/make_pyin_golden.py`` writes ``tests/golden/pyin.npz`` from the unmodified reference; the host tests
(``test_pyin_host.py``) and the device tests (``test_pyin_gpu.py``) share everything here.

(a) The observation kernel alone: float64 CMND in, ``log(observation_probs + tiny)`` and ``voiced_prob`` out, against the reference's
    ``__pyin_helper`` on the same numbers.  The two real CMND arrays are stored in the golden file (an FFT's bits are the machine's); the shifts are
    recomputed from them (additions and one division: every machine's bits) and the synthetic rows come from a seed, both under a SHA-256 digest.
    Every trough test and every ``h < t_j`` is exact on both sides; a candidate's bin is *settled* when its value before rounding lies more than
    ``HALF_MARGIN`` from a half (device log2 error at values up to 600: about 1e-13), and every case must have every candidate settled.
(b) The decode glue: ``pyin`` against the NumPy Viterbi model of ``viterbi_cases`` run on the downloaded ``_pyin_log_prob`` table, bit for bit.
(c) End to end against the reference's ``pyin``; the generator certifies every case (see ``certify``).
(d) Refusals with the reference's text where it has one.
"""
import hashlib
import json
import os

import numpy as np

import yin_cases as YC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pyin.npz")
SR = 22050
HALF_MARGIN = 1e-9
ULP = 2.0**-52
TINY = np.finfo(np.float64).tiny
C2, C7 = 65.40639132514966, 2093.004522404789   # note_to_hz("C2"), note_to_hz("C7")

# the observation cases share one analysis: 130 lags (two rounds of 64 and a tail), periods 18 .. 147; the last lag lies below fmin and the
# first rounds to bin P
OBS_KW = dict(sr=SR, fmin=150.5, fmax=1200.0, frame_length=512, hop_length=128)
OBS_DEFAULTS = dict(n_thresholds=100, beta_parameters=(2, 18), boltzmann_parameter=2, resolution=0.1, no_trough_prob=0.01)


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


# ---- signals ------------------------------------------------------------------------------------------------------------------------------------
def make_signal(kind, n, seed, lead=(), dtype="float64", sr=SR, f_lo=330.0, f_hi=520.0):
    rng = np.random.default_rng(seed)
    shape = lead + (n,)
    t = np.arange(n) / sr
    if kind == "tone_gap":   # a gliding tone with a noise gap in the middle third
        lo = f_lo * (1.0 + 0.1 * rng.random(lead + (1,)))
        phase = 2 * np.pi * (lo * t + 0.5 * (f_hi - f_lo) / t[-1] * t * t)
        y = 0.4 * (np.sin(phase) + 0.5 * np.sin(2 * phase + 0.3) + 0.25 * np.sin(3 * phase + 1.1)) + 0.004 * rng.standard_normal(shape)
        y[..., n // 3: 2 * n // 3] = 0.2 * rng.standard_normal(shape)[..., n // 3: 2 * n // 3]
    elif kind == "noise":
        y = 0.3 * rng.standard_normal(shape)
    elif kind == "zeros":
        y = np.zeros(shape)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(y.astype(dtype))


# ---- the model of the observation stage, line by line (core/pitch.py:796-825, 855-931) ---------------------------------------------------------------
def bins(fmin, fmax, resolution):
    n_bins_per_semitone = int(np.ceil(1.0 / resolution))
    return n_bins_per_semitone, int(np.floor(12 * n_bins_per_semitone * np.log2(fmax / fmin))) + 1


def prior(n_thresholds, beta_parameters):
    import scipy.stats

    thresholds = np.linspace(0, 1, n_thresholds + 1)
    beta_cdf = scipy.stats.beta.cdf(thresholds, beta_parameters[0], beta_parameters[1])
    return thresholds, np.diff(beta_cdf)


def helper_model(yin_frames, parabolic_shifts, sr, thresholds, boltzmann_parameter, beta_probs, no_trough_prob, min_period, fmin, n_pitch_bins, n_bins_per_semitone):
    """``__pyin_helper`` of one clip (n_lags, n_frames): (observation_probs (2 P, T), voiced_prob (T,), info) with info: the smallest distance of a
    candidate's bin value from a half, and the events met."""
    import scipy.stats

    yin_probs = np.zeros_like(yin_frames)
    ev = set()
    for i, yin_frame in enumerate(yin_frames.T):
        is_trough = YC.localmin(yin_frame[:, None])[:, 0]
        is_trough[0] = yin_frame[0] < yin_frame[1]
        (trough_index,) = np.nonzero(is_trough)
        if len(trough_index) == 0:
            ev.add("no_trough")
            continue
        trough_heights = yin_frame[trough_index]
        trough_thresholds = np.less.outer(trough_heights, thresholds[1:])
        trough_positions = np.cumsum(trough_thresholds, axis=0) - 1
        n_troughs = np.count_nonzero(trough_thresholds, axis=0)
        with np.errstate(all="ignore"):
            trough_prior = scipy.stats.boltzmann.pmf(trough_positions, boltzmann_parameter, n_troughs)
        trough_prior[~trough_thresholds] = 0
        probs = trough_prior.dot(beta_probs)
        global_min = np.argmin(trough_heights)
        n_thresholds_below_min = np.count_nonzero(~trough_thresholds[global_min, :])
        probs[global_min] += no_trough_prob * np.sum(beta_probs[:n_thresholds_below_min])
        yin_probs[trough_index, i] = probs
        if is_trough[0]:
            ev.add("first_lag")
        if is_trough[-1]:
            ev.add("last_lag")
        if len(trough_index) > 64:
            ev.add("over_64_troughs")
        if np.isin(trough_heights, thresholds[1:]).any():
            ev.add("height_equals_threshold")
        if (trough_heights < 0.01).any():
            ev.add("below_0.01")
    yin_period, frame_index = np.nonzero(yin_probs)
    period_candidates = min_period + yin_period
    period_candidates = period_candidates + parabolic_shifts[yin_period, frame_index]
    f0_candidates = sr / period_candidates
    bin_index = 12 * n_bins_per_semitone * np.log2(f0_candidates / fmin)
    half = float(np.min(np.abs(bin_index - np.floor(bin_index) - 0.5), initial=np.inf))
    if (bin_index < 0).any():
        ev.add("below_fmin")
    bin_index = np.clip(np.round(bin_index), 0, n_pitch_bins).astype(int)
    if (bin_index == n_pitch_bins).any():
        ev.add("bin_P_dropped")
    if len(set(zip(bin_index.tolist(), frame_index.tolist()))) < len(bin_index):
        ev.add("two_in_one_bin")
    observation_probs = np.zeros((2 * n_pitch_bins, yin_frames.shape[1]))
    observation_probs[bin_index, frame_index] = yin_probs[yin_period, frame_index]
    voiced_prob = np.clip(np.sum(observation_probs[:n_pitch_bins, :], axis=0, keepdims=True), 0, 1)
    observation_probs[n_pitch_bins:, :] = (1 - voiced_prob) / n_pitch_bins
    return observation_probs, voiced_prob[0], dict(half=half, events=ev)


def obs_params(kw):
    """The keyword arguments of ``_pyin_log_prob`` / the positional ones of ``__pyin_helper`` for an analysis ``kw`` (OBS_KW with overrides)."""
    p = dict(OBS_DEFAULTS)
    p.update({k: v for k, v in kw.items() if k in OBS_DEFAULTS})
    sr, fmin, fmax = kw.get("sr", SR), kw["fmin"], kw["fmax"]
    min_period = int(np.floor(sr / fmax))
    nb, P = bins(fmin, fmax, p["resolution"])
    return dict(sr=sr, fmin=fmin, fmax=fmax, min_period=min_period, **p), nb, P


def obs_model(cmnd, shifts, kw):
    """The model over the leading dimensions: (probs (..., 2 P, T), voiced_prob (..., T), info)."""
    p, nb, P = obs_params(kw)
    thresholds, beta_probs = prior(p["n_thresholds"], p["beta_parameters"])
    lead = cmnd.shape[:-2]
    flat_c, flat_s = cmnd.reshape((-1,) + cmnd.shape[-2:]), shifts.reshape((-1,) + shifts.shape[-2:])
    out = [helper_model(c, s, p["sr"], thresholds, p["boltzmann_parameter"], beta_probs, p["no_trough_prob"], p["min_period"], p["fmin"], P, nb) for c, s in zip(flat_c, flat_s)]
    info = dict(half=min(o[2]["half"] for o in out), events=set().union(*(o[2]["events"] for o in out)))
    return np.stack([o[0] for o in out]).reshape(lead + out[0][0].shape), np.stack([o[1] for o in out]).reshape(lead + out[0][1].shape), info


# ---- (a) the observation cases --------------------------------------------------------------------------------------------------------------------
N_LAGS = 130
SOURCES = {"tone": ("tone_gap", 65, 11), "noise": ("noise", 64, 12)}   # kind, frames, seed: the stored CMND arrays


def source_signal(src):
    kind, frames, seed = SOURCES[src]
    return make_signal(kind, (frames - 1) * OBS_KW["hop_length"], seed)


def synthetic_rows():
    """(N_LAGS, 24) crafted CMND rows; ``obs_model`` reports the events, which the generator and the host tests assert."""
    rng = np.random.default_rng(5)
    n, T = N_LAGS, 24
    c = 1.0 + 0.5 * rng.random((n, T))
    thresholds = np.linspace(0, 1, 101)
    c[:, 0] = 1.0                                   # a constant row: no trough
    c[0, 1] = 0.3                                   # a trough at the first lag: f0 above fmax, bin P, dropped
    c[n - 1, 2] = 0.2                               # a trough at the last lag: below fmin, bin 0
    c[:, 3] = 1.5
    c[1::2, 3] = 0.5 + 0.3 * rng.random(n // 2)     # 65 troughs
    c[40, 4] = thresholds[30]                       # a height that equals a threshold (h < t_j is strict)
    c[41, 4], c[39, 4] = 1.2, 1.3
    c[50, 5] = 0.005                                # a trough below 0.01
    c[100:129, 6] = 1.4
    c[120, 6], c[122, 6], c[124, 6], c[126, 6] = 0.11, 0.12, 0.13, 0.14   # neighbouring long periods: one bin at resolution 0.5
    c[:, 7:] = 1.5 * rng.random((n, T - 7))         # dense random rows: many troughs, many shared bins
    return np.ascontiguousarray(c)


OBS_CASES = {
    "tone65": dict(src="tone", frames=65),
    "noise64": dict(src="noise", frames=64),
    "noise64_r05": dict(src="noise", frames=64, resolution=0.5),
    "syn": dict(src="syn", frames=24),
    "syn_r05": dict(src="syn", frames=24, resolution=0.5),
    "noise_thr1": dict(src="noise", frames=16, n_thresholds=1),
    "noise_thr130": dict(src="noise", frames=16, n_thresholds=130),
    "noise_boltz05": dict(src="noise", frames=16, boltzmann_parameter=0.5),
    "noise_notrough0": dict(src="noise", frames=16, no_trough_prob=0),
    "noise_1": dict(src="noise", frames=1),
    "tone_63": dict(src="tone", frames=63),
    "noise_lead23": dict(src="noise", frames=10, lead=(2, 3)),
}
SYN_EVENTS = {"no_trough", "first_lag", "last_lag", "over_64_troughs", "height_equals_threshold", "below_0.01", "below_fmin", "bin_P_dropped", "two_in_one_bin"}


def obs_kw(name):
    c = OBS_CASES[name]
    return dict(OBS_KW, **{k: v for k, v in c.items() if k in OBS_DEFAULTS})


def obs_inputs(name, arrays):
    """(cmnd, shifts) float64 (..., N_LAGS, frames) of a case; ``arrays``: the golden file's (the stored CMND arrays)."""
    c = OBS_CASES[name]
    full = synthetic_rows() if c["src"] == "syn" else arrays["cmnd_" + c["src"]]
    lead, T = c.get("lead", ()), c["frames"]
    count = int(np.prod(lead)) if lead else 1
    cm = np.stack([full[:, i * T:(i + 1) * T] for i in range(count)]).reshape(lead + (N_LAGS, T))
    cm = np.ascontiguousarray(cm, dtype=np.float64)
    return cm, YC.parabolic_shifts(cm)


def obs_bounds(name):
    """The derived bounds of the issue for a case: (voiced log, voiced_prob absolute)."""
    n_thr = obs_kw(name).get("n_thresholds", 100)
    return (n_thr + 8) * ULP, (n_thr + N_LAGS) * ULP


def check_obs(log_dev, vp_dev, p_ref, vp_ref, n_thresholds, n_lags, report=None):
    """The four checks of (a) on (..., 2 P, T) tables; returns the worst figures relative to their bounds."""
    P = p_ref.shape[-2] // 2
    log_tiny = np.log(0.0 + TINY)
    voiced_dev, voiced_ref = log_dev[..., :P, :], p_ref[..., :P, :]
    zero = voiced_ref == 0
    assert np.array_equal(voiced_dev[zero], np.full(int(zero.sum()), log_tiny)), "a zero probability must store log(tiny) bit for bit"
    want = np.log(voiced_ref[~zero] + TINY)
    err = np.abs(voiced_dev[~zero] - want)
    bound = (n_thresholds + 8) * ULP + 2 * np.spacing(np.abs(want))
    vp_bound = (n_thresholds + n_lags) * ULP
    vp_err = np.abs(vp_dev - vp_ref)
    u_ref = p_ref[..., P:, :]
    u_err = np.abs(np.exp(log_dev[..., P:, :]) - u_ref)
    u_bound = 2 * vp_bound / P + 4 * ULP * u_ref
    worst = dict(voiced=float(np.max(err / bound, initial=0)), voiced_abs=float(np.max(err, initial=0)), voiced_prob=float(np.max(vp_err, initial=0)), vp_bound=vp_bound,
                 unvoiced=float(np.max(u_err / u_bound, initial=0)), unvoiced_abs=float(np.max(u_err, initial=0)), candidates=int((~zero).sum()))
    if report:
        report(worst)
    assert (err <= bound).all(), worst
    assert (vp_err <= vp_bound).all(), worst
    assert (u_err <= u_bound).all(), worst
    # exact ties stay ties: one value over the unvoiced states of a frame
    assert np.array_equal(log_dev[..., P:, :], np.broadcast_to(log_dev[..., P:P + 1, :], u_ref.shape))
    return worst


# ---- (b) the decode glue ----------------------------------------------------------------------------------------------------------------------------
GLUE_CASES = {
    "s24": dict(kw=dict(fmin=300.0, fmax=580.0, frame_length=256, hop_length=64, resolution=1.0), n=4000, states=24, none=True),
    "s50": dict(kw=dict(fmin=150.5, fmax=610.0, frame_length=512, hop_length=128, resolution=1.0), n=6000, states=50, none=True),
    "s242": dict(kw=dict(fmin=300.0, fmax=601.5, frame_length=256, hop_length=64), n=4000, states=242, none=False),
    "s1202": dict(kw=dict(fmin=C2, fmax=C7 + 0.1, frame_length=2048, hop_length=512), n=8192, states=1202, none=False),
}


def glue_signal(name):
    return make_signal("tone_gap", GLUE_CASES[name]["n"], 21, f_lo=320.0, f_hi=480.0)


def transition_tables(core_sequence, kw, hop, sr=SR, max_transition_rate=35.92, switch_prob=0.01):
    """The reference's transition and p_init (core/pitch.py:827-839) from the package's builders (equal to the reference's: test_viterbi_host)."""
    nb, P = bins(kw["fmin"], kw["fmax"], kw.get("resolution", 0.1))
    width = round(max_transition_rate * 12 * hop / sr) * nb + 1
    transition = np.kron(core_sequence.transition_loop(2, 1 - switch_prob), core_sequence.transition_local(P, width, window="triangle", wrap=False))
    return transition, np.ones(2 * P) / (2 * P), nb, P


def model_decode(log_prob, transition, p_init, transition_min_prob):
    """states (..., T) of the NumPy Viterbi model of viterbi_cases on a log table (..., S, T)."""
    import viterbi_cases as VC

    thr = np.log(transition_min_prob + TINY) if transition_min_prob else -np.inf
    lt, lpi = np.log(transition + TINY), np.log(p_init + TINY)
    flat = log_prob.reshape((-1,) + log_prob.shape[-2:])
    return np.stack([VC.model(x, lt, lpi, thr)[0] for x in flat]).reshape(log_prob.shape[:-2] + log_prob.shape[-1:])


def lookup(states, kw, fill_na):
    """core/pitch.py:844-850."""
    nb, P = bins(kw["fmin"], kw["fmax"], kw.get("resolution", 0.1))
    freqs = kw["fmin"] * 2 ** (np.arange(P) / (12 * nb))
    f0 = freqs[states % P]
    voiced_flag = states < P
    if fill_na is not None:
        f0[~voiced_flag] = fill_na
    return f0, voiced_flag


# ---- (c) end to end ---------------------------------------------------------------------------------------------------------------------------------
_K242 = dict(sr=SR, fmin=300.0, fmax=601.5, frame_length=256, hop_length=64)
E2E_CASES = {
    "e_tone_gap": dict(kind="tone_gap", n=6000, seed=31, kw=_K242),
    "e_noise": dict(kind="noise", n=4000, seed=32, kw=_K242),
    "e_zeros": dict(kind="zeros", n=3000, seed=33, kw=_K242),
    "e_default": dict(kind="tone_gap", n=11025, seed=34, kw=dict(sr=SR, fmin=C2, fmax=C7 + 0.1)),
    "e_nocenter": dict(kind="tone_gap", n=4000, seed=35, kw=dict(_K242, center=False)),
    "e_reflect": dict(kind="tone_gap", n=4000, seed=36, kw=dict(_K242, pad_mode="reflect")),
    "e_one_frame": dict(kind="tone_gap", n=256, seed=37, kw=dict(_K242, center=False)),
    "e_f32": dict(kind="tone_gap", n=4000, seed=38, dtype="float32", kw=_K242),
    "e_lead23": dict(kind="tone_gap", n=2500, seed=39, lead=(2, 3), kw=_K242),
}
CERT_FACTOR = 4.0
N_PERTURB = 8


def e2e_signal(name):
    c = E2E_CASES[name]
    return make_signal(c["kind"], c["n"], c["seed"], lead=c.get("lead", ()), dtype=c.get("dtype", "float64"))


def e2e_states(name):
    return 2 * bins(E2E_CASES[name]["kw"]["fmin"], E2E_CASES[name]["kw"]["fmax"], 0.1)[1]


def comparison_margin(cmnd, shifts, kw):
    """The smallest distance by which a comparison of the observation stage holds on a CMND (..., n_lags, T): the trough tests, every
    ``h < t_j``, the argmin among the trough heights; frames that are zero throughout are exact on every side and skipped.  Also the smallest
    distance of a candidate's bin value from a half."""
    p, nb, P = obs_params(kw)
    thresholds = np.linspace(0, 1, p["n_thresholds"] + 1)[1:]
    margin = np.inf
    flat = cmnd.reshape((-1,) + cmnd.shape[-2:])
    for clip in flat:
        for frame in clip.T:
            if not frame.any():
                continue
            margin = min(margin, float(np.min(np.abs(np.diff(frame)))))
            is_trough = YC.localmin(frame[:, None])[:, 0]
            is_trough[0] = frame[0] < frame[1]
            h = frame[is_trough]
            if h.size:
                margin = min(margin, float(np.min(np.abs(h[:, None] - thresholds[None, :]))))
            if h.size > 1:
                s = np.sort(h)
                margin = min(margin, float(s[1] - s[0]))
    return margin, obs_model(cmnd, shifts, kw)[2]["half"]


def path_score(states, log_prob, transition, p_init):
    """The log probability of a path (T,) under tables as given (log_prob (S, T))."""
    lt, lpi = np.log(transition + TINY), np.log(p_init + TINY)
    T = states.shape[0]
    return float(lpi[states[0]] + log_prob[states, np.arange(T)].sum() + lt[states[:-1], states[1:]].sum())


# ---- (d) refusals -----------------------------------------------------------------------------------------------------------------------------------
def refusal_calls():
    """name -> (y, kwargs); the golden file holds the reference's text where the reference refuses too (else None)."""
    y = np.zeros(4096)
    return {
        "no_fmin": (y, dict(fmin=None, fmax=2000.0)),
        "fmax_above_nyquist": (y, dict(fmin=100.0, fmax=20000.0)),
        "too_short": (np.zeros(100), dict(fmin=100.0, fmax=2000.0, center=False)),
        "state_limit": (y, dict(fmin=C2, fmax=C7, resolution=0.01)),
        "n_thresholds_zero": (y, dict(fmin=100.0, fmax=2000.0, n_thresholds=0)),
        "n_thresholds_float": (y, dict(fmin=100.0, fmax=2000.0, n_thresholds=10.5)),
    }


OWN_REFUSALS = {"state_limit": "is too large for the device decoder", "n_thresholds_zero": "must be a positive integer", "n_thresholds_float": "must be a positive integer"}


def load():
    z = np.load(GOLDEN)
    arrays = {k: z[k] for k in z.files if k != "meta"}
    return arrays, json.loads(bytes(z["meta"]).decode())


# ---- the checks, shared by the host and the device tests ------------------------------------------------------------------------------------------
def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def run_obs_case(name, pitch, arrays, wrap=lambda a: a, report=None):
    """(a) for one case through ``pitch._pyin_log_prob`` (``wrap``: NumPy array -> what the call is given)."""
    kw = obs_kw(name)
    p, nb, P = obs_params(kw)
    cm, sh = obs_inputs(name, arrays)
    before = cm.copy(), sh.copy()
    log_dev, vp_dev = pitch._pyin_log_prob(wrap(cm), wrap(sh), **p)
    assert np.array_equal(cm, before[0]) and np.array_equal(sh, before[1]), "the inputs were written"
    log_dev, vp_dev = _np(log_dev), _np(vp_dev)
    lead, T = OBS_CASES[name].get("lead", ()), OBS_CASES[name]["frames"]
    assert log_dev.shape == lead + (2 * P, T) and vp_dev.shape == lead + (T,) and log_dev.dtype == vp_dev.dtype == np.float64
    vp_ref = arrays["vp_" + name]
    u = np.broadcast_to(((1 - vp_ref) / P)[..., None, :], lead + (P, T))
    p_ref = np.concatenate([arrays["obs_" + name], u], axis=-2)
    return check_obs(log_dev, vp_dev, p_ref, vp_ref, p["n_thresholds"], N_LAGS, report=report)


def run_glue_case(name, L, transition_min_prob, wrap=lambda a: a):
    """(b) for one case: pyin against the NumPy Viterbi model on the device path's own table, bit for bit, for every fill_na."""
    c = GLUE_CASES[name]
    kw = dict(sr=SR, **c["kw"])
    y = glue_signal(name)
    front = {k: v for k, v in kw.items() if k != "resolution"}
    cm, sh, min_period = L.core.pitch._yin_frames(wrap(y), **front)
    p, nb, P = obs_params(kw)
    assert 2 * P == c["states"] and p["min_period"] == min_period
    log_prob, vp = L.core.pitch._pyin_log_prob(cm, sh, **p)
    log_prob = _np(log_prob)
    transition, p_init, _, _ = transition_tables(L.sequence, kw, kw["hop_length"])
    states = model_decode(log_prob, transition, p_init, transition_min_prob)
    for fill_na in (None, np.nan, 0.0):
        f0, flag, vp2 = L.pyin(wrap(y), fill_na=fill_na, transition_min_prob=transition_min_prob, **kw)
        want_f0, want_flag = lookup(states, kw, fill_na)
        f0, flag = _np(f0), _np(flag)
        assert f0.dtype == np.float64 and flag.dtype == np.bool_ and f0.shape == flag.shape == want_f0.shape
        assert np.array_equal(flag, want_flag), (name, fill_na)
        assert np.array_equal(f0, want_f0, equal_nan=True), (name, fill_na)
        assert np.array_equal(_np(vp2), _np(vp))
    return int(want_flag.sum()), want_flag.size


def run_e2e_case(name, L, arrays, wrap=lambda a: a, report=None, **extra):
    """(c) for one case against the reference's outputs in the golden file; returns pyin's outputs as NumPy arrays."""
    c = E2E_CASES[name]
    y = e2e_signal(name)
    before = y.copy()
    f0, flag, vp = L.pyin(wrap(y), **c["kw"], **extra)
    assert np.array_equal(y, before), "y was written"
    f0, flag, vp = _np(f0), _np(flag), _np(vp)
    want_f0, want_flag, want_vp = arrays["f0_" + name], arrays["flag_" + name], arrays["vp_" + name]
    assert f0.dtype == vp.dtype == np.float64 and flag.dtype == np.bool_ and f0.shape == flag.shape == vp.shape == want_f0.shape
    p, nb, P = obs_params(c["kw"])
    n_lags = YC.periods(c["kw"])[1] - YC.periods(c["kw"])[0] + 1
    vp_bound = (p["n_thresholds"] + n_lags) * ULP
    if report:
        report(dict(name=name, voiced_prob=float(np.max(np.abs(vp - want_vp), initial=0)), vp_bound=vp_bound, flags_differ=int((flag != want_flag).sum())))
    assert np.max(np.abs(vp - want_vp), initial=0) <= vp_bound
    assert np.array_equal(flag, want_flag)
    assert np.array_equal(f0, want_f0, equal_nan=True)
    return f0, flag, vp


def check_e2e_score(name, L, arrays, wrap=lambda a: a):
    """Up to 242 states: the device path's states, scored under the reference's tables, reach the reference path's score minus 2 T 1e-10."""
    c = E2E_CASES[name]
    kw = c["kw"]
    y = e2e_signal(name)
    hop = kw.get("hop_length") or kw.get("frame_length", 2048) // 4
    transition, p_init, nb, P = transition_tables(L.sequence, kw, hop)
    vp_ref = arrays["vp_" + name]
    u = np.broadcast_to(((1 - vp_ref) / P)[..., None, :], vp_ref.shape[:-1] + (P, vp_ref.shape[-1]))
    log_ref = np.log(np.concatenate([arrays["eobs_" + name], u], axis=-2) + TINY)
    ref_states = model_decode(log_ref, transition, p_init, 1e-4)
    # the device path's states: its best guess with fill_na=None names the bin, voiced_flag the half
    f0, flag, _ = L.pyin(wrap(y), fill_na=None, **kw)
    f0, flag = _np(f0), _np(flag)
    freqs = kw["fmin"] * 2 ** (np.arange(P) / (12 * nb))
    dev_states = np.searchsorted(freqs, f0) + np.where(flag, 0, P)
    assert np.array_equal(freqs[dev_states % P], f0)
    T = f0.shape[-1]
    worst = np.inf
    for d, r, lp in zip(dev_states.reshape(-1, T), ref_states.reshape(-1, T), log_ref.reshape((-1,) + log_ref.shape[-2:])):
        gap = path_score(d, lp, transition, p_init) - path_score(r.astype(np.int64), lp, transition, p_init)
        assert gap >= -2 * T * 1e-10, (name, gap)
        worst = min(worst, gap)
    return worst


def check_refusal(name, L, meta):
    import pytest

    y, kw = refusal_calls()[name]
    with pytest.raises(L.ParameterError) as info:
        L.pyin(y, **kw)
    want = meta["refusals"][name]
    if want is not None:
        assert str(info.value) == want
    else:
        assert OWN_REFUSALS[name] in str(info.value)
