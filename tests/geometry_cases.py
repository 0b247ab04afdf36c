"""Launch-geometry cases of the fused power-of-two kernels: plain data, no GPU.

A frame's spectrum or mel column and an output sample of the inverse depend on the input alone, never on which slot, strip or workgroup
computed them: for every ``stft_iters``, ``istft_strip_groups`` and ``xcd_remap`` the result is the default result, bit for bit
(tests/test_launch_geometry_gpu.py on the device, tests/test_launch_geometry_host.py through the host simulator).

One entry per kernel family.  ``sel`` cites the lines of librosa_amd/csrc/lra_api.hip that select the family's kernel, ``fpb`` is the number
of frame slots (forward) or strips (inverse) of one workgroup with the line it was read from in ``fpb_from``.  Lines of lra_api.hip are cited by
named anchor, ``file [tag] [tag]``: the tag stands in a comment on the cited line (tests/test_launch_geometry_host.py checks that each exists).

FPB = NT / TF (lra_fft.h:44-46) with TF = M / R threads per frame, R = 16 (float32: lra_dispatch.h:25-27) or 8 (float64: lra_dispatch.h:28-30) and
NT = max(TF, 64); the mel kernels run the same transform with NT = 256 (lra_dispatch.h:112-115), the many-band form with NT = 128
(lra_dispatch.h:119-122); the producer / consumer kernel has NP = 2 producer slots (lra_api.hip [geo:pc-np], PcLayout::NP)."""
from collections import namedtuple

# ---- geometry values the issue asks for ---------------------------------------------------------------------------------------------
STFT_ITERS = (1, 2, 3, 4, 5, 7, 8, 9, 13, 24)  # + one value above the clip's frame count (forward_points)
ISTFT_STRIPS = (1, 2, 3, 5, 8, 32, 176)        # + one value above n_used (inverse_points)
MAX_FRAMES = 72                                 # clips stay tiny
EDGE_GRIDS = (63, 64, 65, 71, 72)               # 63: last unmapped grid, 64: first mapped one, 65 / 71: padded by 7 / by 1 (lra_api.hip [geo:xcd-pad] [geo:pc-xcd-pad] [geo:istft-xcd-pad])
HOST_ITERS = (1, 3, 5, 8)
HOST_STRIPS = (1, 3, 8)

# what every test puts back in its `finally` block (the library's defaults, lra_internal.h [ctx:defaults])
OPTION_DEFAULTS = dict(stft_iters=0, istft_strip_groups=0, xcd_remap=1, mel_pc=1, mel_runs=1, generic_mel=0, variant=-1, direct=1, istft16=0)

Forward = namedtuple("Forward", "name kind n_fft hop dtype power n_mels opts fpb fpb_from sel sim bar")
Inverse = namedtuple("Inverse", "name n_fft hop dtype opts fpb fpb_from sel sim")

_F32 = "lra_fft.h:44-46 with lra_dispatch.h:25-27 (R = 16, NT = max(TF, 64))"
_F64 = "lra_fft.h:44-46 with lra_dispatch.h:28-30 (R = 8, NT = max(TF, 64))"
_MEL = "lra_fft.h:44-46 with lra_dispatch.h:112-115 (NT = 256)"


def _fwd(name, kind, n_fft, hop, *, dtype="float32", power=2.0, n_mels=0, opts=None, fpb, fpb_from, sel, sim=None, bar=None):
    bar = bar or {"stft": "stft", "power": "power", "mel": "mel"}[kind]
    return Forward(name, kind, n_fft, hop, dtype, power, n_mels, dict(opts or {}), fpb, fpb_from, sel, sim, bar)


def _both(name, n_fft, hop, **kw):
    """The complex and the |X|^2 epilogue of one kernel family."""
    return [_fwd(name + "-complex", "stft", n_fft, hop, **kw), _fwd(name + "-power", "power", n_fft, hop, **kw)]


FORWARD = []
# general ring (RA = 0), float32: a hop that is no whole number of ring rows and no divisor of n_fft
# lra_api.hip [sel:ring] (the default instance; none of [sel:ringrows] [sel:direct] [sel:regring] [sel:v2] applies)
FORWARD += _both("ring-general-f32", 512, 100, fpb=4, fpb_from=_F32, sel="lra_api.hip [sel:ring]", sim=dict(ring_aligned=0, v2=0))
# ... float64: ring_rows_aligned is consulted for float32 only (lra_api.hip [sel:ringrows-f32])
FORWARD += _both("ring-general-f64", 512, 128, dtype="float64", fpb=2, fpb_from=_F64, sel="lra_api.hip [sel:ring] [sel:ringrows-f32]", sim=dict(ring_aligned=0, v2=0))
# row-aligned ring (RA = 1) with four slots per wave: the rot_uniform path (lra_api.hip [geo:rot-uniform]).  At n_fft = 512 the register ring
# (lra_api.hip [sel:regring]) takes hop n_fft / 4 by default, so the family is reached with the context option direct = 0 (same line)
# -- and, with every option at its default, by the mel families "mel-many", "mel-masked" and "mel-generic" below (hop n_fft / 4).
FORWARD += _both("ring-rows-n512", 512, 128, opts=dict(direct=0), fpb=4, fpb_from=_F32, sel="lra_api.hip [sel:ringrows-f32] [sel:ringrows] ([sel:regring]: direct = 0)")
# direct framing (RA = 2): hop >= n_fft
FORWARD += _both("direct-n512", 512, 640, fpb=4, fpb_from=_F32, sel="lra_api.hip [sel:direct]", sim=dict(v2=0))
# register ring (RA = 3 .. 6): n_fft = 8192 with hop n_fft / 2, / 4, / 8, / 16; and the four-slot form at n_fft = 512
for _hd in (2, 4, 8, 16):
    FORWARD += _both(f"regring-n8192-hd{_hd}", 8192, 8192 // _hd, fpb=1, fpb_from=_F32, sel="lra_api.hip [sel:regring]", sim=dict(v2=0) if _hd == 4 else None)
FORWARD += _both("regring-n512-hd4", 512, 128, fpb=4, fpb_from=_F32, sel="lra_api.hip [sel:regring]", sim=dict(v2=0))
# stft2_kernel, HD = 1, 2, 4, 8 at n_fft = 1024 (two slots per wave) and 4096 (two waves per frame)
for _hd in (1, 2, 4, 8):
    FORWARD += _both(f"stft2-n1024-hd{_hd}", 1024, 1024 // _hd, fpb=2, fpb_from=_F32, sel="lra_api.hip [sel:v2]", sim=dict(v2=1))
    FORWARD += _both(f"stft2-n4096-hd{_hd}", 4096, 4096 // _hd, fpb=1, fpb_from=_F32, sel="lra_api.hip [sel:v2]", sim=dict(v2=1) if _hd == 4 else None)
# n_fft = 2048: the complex epilogue runs in the radix 16-16-4 form (variant 6), |X|^2 in stft2_kernel on the 16-8-8 core
FORWARD += [_fwd(f"radix-16-16-4-hd{_hd}-complex", "stft", 2048, 2048 // _hd, fpb=1, fpb_from=_F32, sel="lra_api.hip [sel:v2-applies] [sel:variant-fwd] (variant 6) [sel:plan1] [sel:v2]")
            for _hd in (4, 8)]
FORWARD += [_fwd("stft2-n2048-hd4-power", "power", 2048, 512, fpb=1, fpb_from=_F32, sel="lra_api.hip [sel:variant-fwd] (variant 0) [sel:v2]", sim=dict(v2=1))]

# ---- fused mel --------------------------------------------------------------------------------------------------------------------
_PC = "lra_api.hip [geo:pc-np] (PcLayout::NP = 2)"
FORWARD += [
    # stft_pc_kernel: HD = 4 serves |X|^2, HD = 8 serves |X| and |X|^2 (pc_fits_budget); 128 and 125 bands
    _fwd(f"mel-pc-hd{4 if hop == 512 else 8}-p{int(p)}-{nm}", "mel", 2048, hop, power=p, n_mels=nm, fpb=2, fpb_from=_PC, sel="lra_api.hip [sel:mel-pc] [sel:launch-pc]", bar="mel-rel")
    for hop, p in ((512, 2.0), (256, 1.0), (256, 2.0)) for nm in (128, 125)
]
FORWARD += [
    # the one-wave run-ordered kernel, stft2_kernel<OUT_MELR> in 256-thread workgroups
    _fwd("mel-onewave", "mel", 2048, 512, n_mels=128, opts=dict(mel_pc=0), fpb=4, fpb_from=_MEL, sel="lra_api.hip [sel:mel-onewave] ([sel:mel-pc]: mel_pc = 0)", bar="mel-rel"),
    # the many-band small-frame form: n_fft = 512 with more than 100 bands, eight slots of sixteen threads
    _fwd("mel-many", "mel", 512, 128, n_mels=128, fpb=8, fpb_from="lra_fft.h:44-46 with lra_dispatch.h:119-122 (NT = 128)", sel="lra_api.hip [sel:mel-many] [sel:mel-many-plan]"),
    # the masked two-slope fallback; staging tile 4 (lra_api.hip [geo:staging-tile]), so stft_iters 1 .. 3 exercise the clamp mel_tile = iters (lra_api.hip [geo:mel-tile])
    _fwd("mel-masked", "mel", 2048, 512, n_mels=128, opts=dict(mel_runs=0), fpb=4, fpb_from=_MEL, sel="lra_api.hip [sel:mel-masked] ([sel:mel-pc] [sel:mel-onewave] [sel:mel-runs]: mel_runs = 0)"),
    # the generic banded path; staging tile 4 (lra_api.hip [geo:mel-tile])
    _fwd("mel-generic", "mel", 2048, 512, n_mels=128, opts=dict(generic_mel=1), fpb=1, fpb_from=_F32, sel="lra_api.hip [sel:generic-mel-option] (generic_mel = 1) [sel:mel-generic]"),
]
STAGING_TILE = 4  # lra_api.hip [geo:mel-tile] [geo:staging-tile]: the two staged mel families run with stft_iters below it

# ---- inverse ----------------------------------------------------------------------------------------------------------------------
INVERSE = [
    # istft_kernel<Cfg, 0>: a hop that is no whole number of rows (n_fft = 2048: lra_api.hip [sel:istft-mixed-pow2] sends 256 / 512 / 1024 to another kernel), and float64
    Inverse("general-f32", 2048, 300, "float32", {}, 1, _F32, "lra_api.hip [sel:istft-general] (no form of [sel:istft-rows]) [sel:variant-inv] (variant 0)", None),
    Inverse("general-f64", 512, 128, "float64", {}, 2, _F64, "lra_api.hip [sel:istft-general] [sel:istft-rows] (row forms are float32 only)", dict(ring_aligned=0)),
]
# the row-aligned forms HC = R / 2, R / 4, R / 8, R / 16 with four strips per workgroup
INVERSE += [Inverse(f"rows-n512-hc-r{d}", 512, 512 // d, "float32", {}, 4, _F32, "lra_api.hip [sel:istft-rows]", dict(ring_aligned=1)) for d in (2, 4, 8, 16)]
INVERSE += [
    # n_fft = 2048, hop n_fft / 4: radices 8, 8, 16 by default (variant 5), radices 4, 16, 16 with istft16 = 1 (variant 7)
    Inverse("n2048-8-8-16", 2048, 512, "float32", {}, 1, _F32, "lra_api.hip [sel:variant-inv] (variant 5) [sel:istft-plan1] [sel:istft-rows]", None),
    Inverse("n2048-4-16-16", 2048, 512, "float32", dict(istft16=1), 1, _F32, "lra_api.hip [sel:variant-inv] (variant 7) [sel:istft-plan1] [sel:istft-rows]", None),
    Inverse("n2048-4-16-16-hd8", 2048, 256, "float32", dict(istft16=1), 1, _F32, "lra_api.hip [sel:variant-inv] (variant 7) [sel:istft-plan1] [sel:istft-rows]", None),
]

FORWARD_BY_NAME = {f.name: f for f in FORWARD}
INVERSE_BY_NAME = {f.name: f for f in INVERSE}
assert len(FORWARD_BY_NAME) == len(FORWARD) and len(INVERSE_BY_NAME) == len(INVERSE)

# stft_pc_kernel: the simulator's own (n_frames, iters) pairs of tests/test_pc_tile_phases.py and tests/test_pc_producer_paths.py, unchanged
# (kept as literals here so that this module stays plain data; tests/test_launch_geometry_host.py asserts they are those modules' lists)
PC_TILE_PHASE_PAIRS = [(16, 3), (17, 5), (18, 9), (19, 10), (20, 11), (21, 6), (22, 13), (23, 7)]
PC_PRODUCER_PAIRS = [(nf, it) for nf in (1, 2, 3, 5) for it in (1, 2, 3)]


def n_samples(n_frames, hop):
    """A centred clip of exactly n_frames frames (1 + n // hop) whose last hop is partly filled."""
    return (n_frames - 1) * hop + min(37, hop - 1)


def forward_points(fpb, iters_list=STFT_ITERS, above=True):
    """[(n_frames, iters)]: for every iters, clips whose last workgroup is full, holds one frame, and whose last slot lies wholly past the
    clip (one slot per workgroup: a slot that is cut short instead); plus one iters above the clip's frame count."""
    pts = []
    for it in iters_list:
        w = fpb * it  # frames of one workgroup
        if w <= MAX_FRAMES:
            k = MAX_FRAMES // w if w > 8 else max(1, 24 // w)  # (short slots: a few workgroups are enough)
            full = k * w
            one = full + 1 if full + 1 <= MAX_FRAMES + 1 else (k - 1) * w + 1
            past = (k - 1) * w + ((fpb - 1) * it if fpb > 1 else max(1, it // 2))
            cands = [full, one, past]
        else:  # one workgroup is longer than any clip here: slot 0 full and the others wholly past; slot 1 with one frame; a cut slot
            cands = [it, it + 1, MAX_FRAMES - 2]
        for nf in cands:
            if nf >= 1 and (nf, it) not in pts:
                pts.append((nf, it))
    if above:
        pts += [(1, 2), (5, 9), (23, 40)]  # iters above the clip's frame count
    return pts


def inverse_points(fpb, strips_list=ISTFT_STRIPS, above=True):
    """[(n_used, strips, batch)]: the last strip whole, the last strip one frame, and (batch 3, a strip count per clip that is no multiple
    of FPB) a workgroup whose FPB strips straddle two clips; plus one strip length above n_used."""
    pts = []
    for sf in strips_list:
        if sf <= MAX_FRAMES // 2:
            k = max(2, min(5, MAX_FRAMES // sf)) if sf > 1 else 7
            if fpb > 1 and k % fpb == 0:
                k += 1  # strips per clip no multiple of FPB: with three clips some workgroup serves two clips
            cands = [k * sf, (k - 1) * sf + 1]
        else:
            cands = [min(sf, MAX_FRAMES), MAX_FRAMES // 2 + 1] if sf <= MAX_FRAMES else [MAX_FRAMES, 9]
        for nu in cands:
            if (nu, sf, 3) not in pts:
                pts.append((nu, sf, 3))
    if above:
        pts += [(2, 4, 3), (7, 11, 3)]  # (two frames at least: without `length` one centred frame reaches no sample)
    return pts


def straddles(n_used, strips, batch, fpb):
    """True where some workgroup's FPB strips belong to two clips (lra_kernels.h: istft_slot)."""
    spc = -(-n_used // strips)
    total = batch * spc
    return any((b * fpb) // spc != (min(b * fpb + fpb, total) - 1) // spc for b in range(-(-total // fpb)))


# ---- grid edge --------------------------------------------------------------------------------------------------------------------
EDGE_ITERS = 2    # forward: clips of EDGE_ITERS frames and stft_iters = EDGE_ITERS -> one workgroup per clip for any FPB: the grid is the batch
EDGE_STRIPS = 3   # inverse: clips of EDGE_STRIPS frames and istft_strip_groups = EDGE_STRIPS -> one strip per clip: the grid is ceil(batch / FPB)


def forward_grid(batch, n_frames, iters, fpb):
    """StftLaunch::launch / launch_pc: lra_api.hip [geo:strips] [geo:pc-strips]."""
    return batch * -(-n_frames // (fpb * iters))


def inverse_grid(batch, n_used, strips, fpb):
    """IstftLaunch::run: lra_api.hip [geo:istft-strips]."""
    return -(-(batch * -(-n_used // strips)) // fpb)


def launched(grid, xcd_remap=1):
    """Workgroups launched for `grid` work items: padded to a multiple of 8 from 64 on (lra_api.hip [geo:xcd-pad])."""
    return -(-grid // 8) * 8 if (xcd_remap and grid >= 64) else grid


def edge_batches_forward():
    return list(EDGE_GRIDS)


def edge_batches_inverse(fpb):
    """Batches whose grids are EDGE_GRIDS under `fpb` strips per workgroup; the last workgroup holds one strip (the others of its slots are
    past the batch) except where that would repeat a batch."""
    return [(g - 1) * fpb + 1 for g in EDGE_GRIDS]


# families that run the grid edge, the many-round and the auto-rule cases on the device
EDGE_FORWARD = ("ring-general-f32-complex", "ring-rows-n512-power", "regring-n512-hd4-complex", "stft2-n1024-hd4-complex", "radix-16-16-4-hd4-complex", "stft2-n2048-hd4-power",
                "mel-pc-hd4-p2-128", "mel-pc-hd8-p1-125", "mel-onewave", "mel-many", "mel-masked", "mel-generic")
EDGE_INVERSE = ("general-f64", "rows-n512-hc-r4", "rows-n512-hc-r16", "n2048-8-8-16", "n2048-4-16-16")
ROUNDS_FORWARD = ("stft2-n1024-hd4-complex", "mel-pc-hd4-p2-128")
ROUNDS_INVERSE = ("rows-n512-hc-r4",)
ROUNDS_FRAMES = 24        # frames per clip in the many-round cases
WAVE_SLOTS_PER_CU = 32    # an upper bound on the resident workgroups per CU for any of these kernels: 4 SIMDs x 8 waves


def rounds_batch(n_cu, fpb, inverse=False):
    """Clips of ROUNDS_FRAMES frames so that, with one frame per slot (strip), the grid is at least three times n_cu * WAVE_SLOTS_PER_CU."""
    per_clip = ROUNDS_FRAMES / fpb if inverse else -(-ROUNDS_FRAMES // fpb)
    return int(-(-(3 * n_cu * WAVE_SLOTS_PER_CU) // per_clip))


def auto_rule_batch(n_cu):
    """Fused mel under the auto rule: one workgroup per 9 000-sample clip, 1.25 rounds of four resident workgroups per CU."""
    return 5 * n_cu + 3


AUTO_RULE_SAMPLES = 9000
