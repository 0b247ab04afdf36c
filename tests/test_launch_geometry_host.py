"""Launch-geometry invariance through the host simulator, and the case list's own consistency (tests/geometry_cases.py).

The simulator runs the kernels' own bodies (tests/hostsim/hostsim.cpp), so where the device disagrees with itself between two geometries
this file says whether the kernel's logic is wrong or only its compiled form: a family's result for every ``iters_per_wg`` /
``strip_groups`` is its result at one frame per slot / one frame per strip, bit for bit, with no LDS race and no read of unwritten LDS.

No family differs between two geometries in the simulator.  The inverse's overlap-add has no geometry-dependent order of additions either: a strip
starts from a zero carry and replays the ceil(n_fft / hop) - 1 frames before its own (lra_kernels.h: istft_block, `t = s.t0 - a.warm_frames + j`), so an
output sample is always 0 + its frames' contributions in ascending frame order."""
import functools
import os
import re

import numpy as np
import pytest

import geometry_cases as G
import hostsim_util as H
import stft_oracle as O

SR = 22050


def _check_diag(d):
    assert d["races"] == 0 and d["uninit"] == 0, d


def _signal(batch, n, dtype, seed):
    return np.random.default_rng(seed).standard_normal((batch, n)).astype(dtype)


# ---- forward --------------------------------------------------------------------------------------------------------------------------
def _sim_selection(fam):
    """What selects the family in the simulator: (mode, environment, variant), as hostsim.cpp reads them."""
    env = {}
    if fam.opts.get("direct") == 0:
        env["LRA_SIM_NO_DIRECT"] = "1"
    if fam.name.startswith("mel-pc"):
        env["LRA_SIM_PC"] = "1"
    mode = {"stft": 0, "power": 1}.get(fam.kind)
    if mode is None:
        mode = {"mel-masked": 3, "mel-generic": 2}.get(fam.name, 4)
    return mode, env, 6 if fam.name.startswith("radix-16-16-4") else 0


_SIM_ENV = ("LRA_SIM_NO_DIRECT", "LRA_SIM_PC", "LRA_SIM_NO_RA", "LRA_SIM_NO_V2", "LRA_SIM_NO_MELMANY")


def _sim_forward(fam, y, iters, monkeypatch):
    mode, env, variant = _sim_selection(fam)
    for k in _SIM_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    win = O.get_window("hann", fam.n_fft)
    B = O.mel(sr=SR, n_fft=fam.n_fft, n_mels=fam.n_mels) if fam.kind == "mel" else None
    out, d = H.stft(y, fam.n_fft, fam.hop, win, mode=mode, power=fam.power, mel_basis=B, iters_per_wg=iters, variant=variant)
    assert out is not None, d
    return out, d


@pytest.mark.parametrize("name", [f.name for f in G.FORWARD])
def test_sim_forward_result_does_not_depend_on_iters(name, monkeypatch):
    fam = G.FORWARD_BY_NAME[name]
    # (frames per clip: no multiple of any FPB * iters here, so the last workgroup is cut and, with several slots, its last slots lie past the clip)
    n_frames = 9 if fam.n_fft >= 2048 else 11
    y = _signal(2, G.n_samples(n_frames, fam.hop), fam.dtype, 7 * fam.n_fft + fam.hop)
    outs = {}
    for it in G.HOST_ITERS:
        out, d = _sim_forward(fam, y, it, monkeypatch)
        _check_diag(d)
        assert d["FPB"] == fam.fpb, (d, fam.fpb_from)
        for key, want in (fam.sim or {}).items():
            assert d[key] == want, (key, d)
        if "mel-pc" in name:
            assert d["NT"] == 192, d
        if name == "mel-many":
            assert d["mel_many"] == 1, d
        assert not np.isnan(out.view(np.float64 if fam.dtype == "float64" else np.float32)).any(), it
        outs[it] = out
    for it in G.HOST_ITERS[1:]:
        assert np.array_equal(outs[it], outs[G.HOST_ITERS[0]]), (name, it)


# ---- inverse --------------------------------------------------------------------------------------------------------------------------
def _sim_inverse_variant(fam):
    """The configuration lra_api.hip [sel:variant-inv] picks: radices 4, 16, 16 with istft16 = 1, else 8, 8, 16 at n_fft = 2048 with a row-aligned hop."""
    if fam.opts.get("istft16"):
        return 7
    return 5 if fam.name == "n2048-8-8-16" else 0


@pytest.mark.parametrize("name", [f.name for f in G.INVERSE])
@pytest.mark.parametrize("use_length", [False, True])
def test_sim_inverse_result_does_not_depend_on_strips(name, use_length):
    fam = G.INVERSE_BY_NAME[name]
    n_frames = 7 if fam.n_fft >= 2048 else 10  # (three clips of 10 frames in strips of 3: four strips per clip, so a workgroup of four serves two clips)
    rt = np.dtype(fam.dtype)
    y = _signal(3, G.n_samples(n_frames, fam.hop), rt, 3 * fam.n_fft + fam.hop)
    D = O.stft(y, n_fft=fam.n_fft, hop_length=fam.hop)
    assert D.shape[-1] == n_frames
    Dn = np.ascontiguousarray(np.swapaxes(D, -1, -2))
    # `length` shorter than the frames reach: the kernel serves fewer frames than the spectrogram holds and cuts the last hop block
    out_len = (n_frames - 3) * fam.hop + 5 if use_length else (n_frames - 1) * fam.hop
    n_used = min(n_frames, -(-(out_len + fam.n_fft) // fam.hop)) if use_length else n_frames
    win = O.get_window("hann", fam.n_fft)
    wss = O.window_sumsquare(window="hann", n_frames=n_used, n_fft=fam.n_fft, hop_length=fam.hop, dtype=rt)[fam.n_fft // 2:]
    wss = O.fix_length(wss, size=out_len)
    outs = {}
    for sf in G.HOST_STRIPS + (n_frames + 2,):
        out, d = H.istft(Dn, fam.n_fft, fam.hop, win, wss, out_len, n_used, strip_groups=sf, variant=_sim_inverse_variant(fam))
        _check_diag(d)
        assert d["FPB"] == fam.fpb, (d, fam.fpb_from)
        for key, want in (fam.sim or {}).items():
            assert d[key] == want, (key, d)
        assert not np.isnan(out).any(), sf
        outs[sf] = out
    for sf in outs:
        assert np.array_equal(outs[sf], outs[G.HOST_STRIPS[0]]), (name, sf)
    if not use_length:
        ref = O.istft(D, hop_length=fam.hop, n_fft=fam.n_fft)
        assert np.abs(outs[1] - ref).max() <= (1e-12 if rt == np.float64 else 4e-6) * max(1.0, np.abs(ref).max()) / np.sqrt(max(wss.min(), 1e-3))


# ---- the case list ----------------------------------------------------------------------------------------------------------------------
def _cited_tags(text):
    """[(file, "[tag]")] of every ``file [tag] [tag] (remark) [tag]`` citation in `text`: a tag belongs to the file named last before it."""
    out, fname = [], None
    for m in re.finditer(r"(lra_\w+\.(?:hip|h))|(\[[a-z]+:[\w-]+\])", text):
        if m.group(1):
            fname = m.group(1)
        else:
            assert fname, text
            out.append((fname, m.group(2)))
    return out


@functools.lru_cache(maxsize=None)
def _csrc(fname):
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "librosa_amd", "csrc", fname)).read()


def test_every_family_has_a_selection_comment_and_an_fpb():
    # every named anchor the case list cites, in a family's entry or in a comment, stands in the file it is cited from
    every = _cited_tags(open(G.__file__).read())
    assert len(every) > 40
    for fname, tag in every:
        assert tag in _csrc(fname), (fname, tag)
    names = set()
    for fam in G.FORWARD + G.INVERSE:
        assert fam.name not in names
        names.add(fam.name)
        cited = _cited_tags(fam.sel)
        assert cited and cited[0][0] == "lra_api.hip", fam.name
        for fname, tag in cited + _cited_tags(fam.fpb_from):
            assert tag in _csrc(fname), (fam.name, fname, tag)
        assert isinstance(fam.fpb, int) and fam.fpb >= 1 and ":" in fam.fpb_from, fam.name
        assert fam.n_fft & (fam.n_fft - 1) == 0, "power-of-two kernels only"
        assert set(fam.opts) <= set(G.OPTION_DEFAULTS), fam.name
    # FPB as lra_fft.h:44-46 derives it
    for fam in G.FORWARD + G.INVERSE:
        r = 8 if fam.dtype == "float64" else 16
        tf = max(1, fam.n_fft // 2 // r)
        nt = max(tf, 64)
        if isinstance(fam, G.Forward) and fam.kind == "mel":
            if fam.name.startswith("mel-pc"):
                assert fam.fpb == 2
                continue
            nt = {"mel-many": 128, "mel-generic": nt}.get(fam.name, 256)
        assert fam.fpb == nt // tf, fam.name
    # the two staged mel families run with frames per slot below their staging tile (the clamp mel_tile = iters)
    assert sum(it < G.STAGING_TILE for it in G.STFT_ITERS) >= 3 and {"mel-masked", "mel-generic"} <= set(G.FORWARD_BY_NAME)
    for need in ("ring-general-f32", "ring-general-f64", "ring-rows-n512", "direct-n512", "regring-n8192-hd2", "regring-n8192-hd4", "regring-n8192-hd8", "regring-n8192-hd16"):
        assert need + "-complex" in G.FORWARD_BY_NAME and need + "-power" in G.FORWARD_BY_NAME
    for n_fft in (1024, 4096):
        for hd in (1, 2, 4, 8):
            assert f"stft2-n{n_fft}-hd{hd}-complex" in G.FORWARD_BY_NAME
    for fam in G.EDGE_FORWARD + G.ROUNDS_FORWARD:
        assert fam in G.FORWARD_BY_NAME
    for fam in G.EDGE_INVERSE + G.ROUNDS_INVERSE:
        assert fam in G.INVERSE_BY_NAME


def test_pc_pairs_are_the_simulator_cases():
    import test_pc_producer_paths as PP
    import test_pc_tile_phases as TP

    assert G.PC_TILE_PHASE_PAIRS == [(nf, it) for nf, it, _ in TP._SIM_CASES]
    assert sorted(set(G.PC_PRODUCER_PAIRS)) == sorted({(nf, it) for nf, it, _, _ in PP._SIM_CASES})


def test_geometry_points_cover_what_they_claim():
    for fpb in (1, 2, 4, 8):
        pts = G.forward_points(fpb)
        for it in G.STFT_ITERS:
            mine = [nf for nf, i in pts if i == it]
            assert mine and all(1 <= nf <= G.MAX_FRAMES + 1 for nf in mine), (fpb, it, mine)
            w = fpb * it
            if w <= G.MAX_FRAMES:
                assert any(nf % w == 0 for nf in mine), ("last workgroup full", fpb, it)
                assert any(nf % w == 1 for nf in mine) or w == 1, ("last workgroup holds one frame", fpb, it)
                if fpb > 1:  # the last slot's first frame, (nf - 1) // w * w + (fpb - 1) * it, is at or past the clip's end
                    assert any(nf % w and (nf - 1) // w * w + (fpb - 1) * it >= nf for nf in mine), ("last slot wholly past the clip", fpb, it)
        assert any(it > nf for nf, it in pts), "an iters above the clip's frame count"
        inv = G.inverse_points(fpb)
        for sf in G.ISTFT_STRIPS:
            mine = [(nu, b) for nu, s, b in inv if s == sf]
            assert any(nu % sf == 0 or sf > G.MAX_FRAMES for nu, _ in mine), ("last strip whole", fpb, sf)
            assert any(nu % sf == 1 or sf == 1 or sf > G.MAX_FRAMES for nu, _ in mine), ("last strip is one frame", fpb, sf)
        assert any(s > nu for nu, s, _ in inv), "a strip length above n_used"
        if fpb > 1:
            assert any(G.straddles(nu, s, b, fpb) for nu, s, b in inv), ("a workgroup whose strips straddle two clips", fpb)


def test_grid_edge_batches_give_the_five_grids():
    for fam in G.FORWARD:
        grids = [G.forward_grid(b, G.EDGE_ITERS, G.EDGE_ITERS, fam.fpb) for b in G.edge_batches_forward()]
        assert tuple(grids) == G.EDGE_GRIDS, fam.name
    for fam in G.INVERSE:
        grids = [G.inverse_grid(b, G.EDGE_STRIPS, G.EDGE_STRIPS, fam.fpb) for b in G.edge_batches_inverse(fam.fpb)]
        assert tuple(grids) == G.EDGE_GRIDS, fam.name
    # 63 is launched as it is, 64 and 72 are whole, 65 and 71 are padded by 7 and by 1; without the map nothing is padded
    assert [G.launched(g) - g for g in G.EDGE_GRIDS] == [0, 0, 7, 1, 0]
    assert [G.launched(g, 0) - g for g in G.EDGE_GRIDS] == [0] * 5
    for n_cu in (64, 256, 304):
        for name in G.ROUNDS_FORWARD:
            fam = G.FORWARD_BY_NAME[name]
            assert G.forward_grid(G.rounds_batch(n_cu, fam.fpb), G.ROUNDS_FRAMES, 1, fam.fpb) >= 3 * n_cu * G.WAVE_SLOTS_PER_CU
        for name in G.ROUNDS_INVERSE:
            fam = G.INVERSE_BY_NAME[name]
            assert G.inverse_grid(G.rounds_batch(n_cu, fam.fpb, inverse=True), G.ROUNDS_FRAMES, 1, fam.fpb) >= 3 * n_cu * G.WAVE_SLOTS_PER_CU
