"""Shared by tests/test_mel_banks_host.py and tests/test_mel_banks_gpu.py: mel filter banks on both sides of every gate of the fused STFT -> mel launch
(csrc/lra_api.hip, StftLaunch::run / stft_run), a NumPy restatement of the table forms those gates read (csrc/lra_mel.h), the white-noise input and the
float64 reference.

Band counts that straddle each gate (declined | served, or the two forms):
  producer / consumer kernel, n_fft 2048 (pair segments in <= 4 pieces of 8 aligned bins, <= 128 bands):
      22050 Slaney full range 118 | 119 and again 123 | 124,   22050 fmax=8000 80 | 81,   129 | 128 bands,   44100 at 128 bands declined (5 pieces)
  run-ordered form, n_fft 2048 (<= 16 pieces of 8 aligned bins):                22050 Slaney full range 24 | 25
  masked two-slope pieces form, n_fft 2048 (<= 15 pieces of 16 aligned bins):   22050 Slaney full range 11 | 12
  eight bands per thread, n_fft 512:                                            100 | 101
  flat-index kernel:                                                            n_fft 256: 55 | 56,   n_fft 128: 39 | 40
"""
import numpy as np

import librosa_amd as L
import stft_oracle as O

BATCH = 3
MELR_PMAX = 16      # csrc/lra_kernels.h
MEL2_PMAX = 15      # csrc/lra_mel.h, build_mel_pieces
PC_PMAX = 4         # csrc/lra_kernels_pc.h, pc_bank_ok
PC_BANDS = 128
MIXED_SIZES = (400, 1764, 240, 1000)  # csrc/lra_mixed_sizes.h; with the ctx option "mixed" at 0 they take the rocFFT path
SIM_MIXED_SIZES = (400, 240, 1000)    # ... of which the simulator instantiates these (tests/hostsim/postsim.cpp)
# float32 (n_fft, hops of the table) whose run-ordered form runs on the second-generation core (lra_kernels2.h: v2_cfg_ok, v2_hop_divisor)
V2_HOPS = {2048: (512, 256), 1024: (256,)}
# (hop, powers) whose producer wave fits its register budget on the default core (lra_kernels_pc.h, pc_fits_budget)
PC_HOP_POWERS = {256: (1.0, 2.0), 512: (2.0,)}

_HTK48 = dict(htk=True, fmin=20, fmax=20000)
_SPEECH = dict(fmin=20, fmax=7600)

# (n_fft, hop, sr, n_mels, filters.mel kwargs)
CASES = [
    # ---- the producer / consumer gate, n_fft = 2048 ----
    (2048, 512, 22050, 127, {}),
    (2048, 256, 22050, 127, {}),
    (2048, 512, 22050, 128, {}),
    (2048, 256, 22050, 128, {}),
    (2048, 512, 22050, 119, {}),                  # smallest served default bank ...
    (2048, 256, 22050, 118, {}),                  # ... and the one below it (5 pieces)
    (2048, 512, 22050, 112, {}),                  # (5 pieces)
    (2048, 256, 22050, 123, {}),                  # not monotonic: 122 and 123 need 5 pieces again ...
    (2048, 512, 22050, 124, {}),                  # ... from 124 on 4
    (2048, 512, 22050, 113, dict(htk=True)),
    (2048, 256, 22050, 97, dict(fmax=8000)),
    (2048, 512, 22050, 81, dict(fmax=8000)),      # its own edge: from 81 on served ...
    (2048, 256, 22050, 80, dict(fmax=8000)),      # ... 80 declined (5 pieces)
    (2048, 512, 16000, 128, _SPEECH),
    (2048, 512, 44100, 128, {}),                  # 5 pieces: declined
    (2048, 512, 22050, 129, {}),                  # over the lane count: declined
    (2048, 256, 22050, 128, dict(norm=None)),
    (2048, 512, 22050, 120, dict(norm=np.inf)),
    # ---- above 128 bands ----
    (2048, 512, 22050, 160, {}),
    (2048, 512, 22050, 229, {}),
    (2048, 512, 22050, 256, {}),
    (2048, 512, 48000, 160, _HTK48),
    (2048, 512, 48000, 229, _HTK48),
    (2048, 512, 48000, 256, _HTK48),              # two empty filters
    (1024, 256, 48000, 160, _HTK48),              # four empty filters
    # ---- few bands ----
    (2048, 512, 22050, 1, {}), (2048, 512, 22050, 2, {}), (2048, 512, 22050, 3, {}), (2048, 512, 22050, 8, {}),
    (1024, 256, 22050, 1, {}), (1024, 256, 22050, 2, {}), (1024, 256, 22050, 3, {}), (1024, 256, 22050, 8, {}),
    (512, 128, 22050, 1, {}), (512, 128, 22050, 2, {}), (512, 128, 22050, 3, {}), (512, 128, 22050, 8, {}),
    (256, 64, 22050, 1, {}), (256, 64, 22050, 2, {}), (256, 64, 22050, 3, {}), (256, 64, 22050, 8, {}),
    (2048, 512, 22050, 11, {}), (2048, 512, 22050, 12, {}),   # the 15-piece limit of the masked form (16-bin runs): 16 | 15 pieces
    (2048, 512, 22050, 24, {}), (2048, 512, 22050, 25, {}),   # the 16-piece limit of the run-ordered form (8-bin runs): 17 | 16 pieces
    # ---- n_fft = 512 ----
    (512, 128, 22050, 100, {}),
    (512, 128, 22050, 101, {}),
    (512, 128, 44100, 128, {}),                   # 11 empty filters
    (512, 128, 22050, 96, dict(htk=True)),        # one empty filter
    # ---- the flat-index gates ----
    (256, 64, 8000, 55, {}), (256, 64, 8000, 56, {}),
    (128, 32, 8000, 39, {}), (128, 32, 8000, 40, {}),
    # ---- mixed radix ----
    (400, 160, 16000, 128, {}),
    (400, 160, 16000, 80, _SPEECH),
    (1764, 441, 44100, 229, {}),
    (240, 80, 8000, 3, {}),
    (1000, 250, 22050, 64, {}),
    # ---- rocFFT path (n_bins > 4097: generic banded product only) ----
    (16384, 4096, 22050, 128, {}),
]


def case_id(case):
    n_fft, hop, sr, n_mels, kw = case
    tail = "".join(f"-{k}{v}" for k, v in sorted(kw.items()))
    return f"{n_fft}-{hop}-{sr}-{n_mels}{tail}"


# banks with empty filters: how many
EMPTY_FILTERS = {case_id(c): k for c, k in (((2048, 512, 48000, 256, _HTK48), 2), ((1024, 256, 48000, 160, _HTK48), 4), ((512, 128, 44100, 128, {}), 11),
                                            ((512, 128, 22050, 96, dict(htk=True)), 1))}


# ... of which filters.mel warns about these, as the reference does: an empty first filter whose lower edge is 0 Hz is exempt (librosa/filters.py:241)
EMPTY_FILTER_WARNS = [k for k in EMPTY_FILTERS if k != case_id((512, 128, 22050, 96, dict(htk=True)))]


def is_pow2(n_fft):
    return n_fft & (n_fft - 1) == 0


POW2_CASES = [c for c in CASES if is_pow2(c[0])]
SIM_MIXED_CASES = [c for c in CASES if c[0] in SIM_MIXED_SIZES]


def basis(case, dtype=np.float32):
    """``L.filters.mel`` of the case, without its empty-filter warning."""
    import warnings

    n_fft, _, sr, n_mels, kw = case
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return L.filters.mel(sr=sr, n_fft=n_fft, n_mels=n_mels, dtype=dtype, **kw)


def empty_rows(B):
    return ~np.any(B != 0, axis=1)


def segment_owner(B):
    """Pair segment of every bin (build_two_slope): bin k on the rising slope of filter m belongs to segment m, on the falling slope to m + 1; -1 where no
    filter covers it.  None where the bank has no two-slope structure."""
    n_mels, n_bins = B.shape
    owner = np.full(n_bins, -1)
    peak = np.argmax(B, axis=1)  # (first maximum, as the builder's strict comparison keeps)
    for k in range(n_bins):
        rows = np.nonzero(B[:, k])[0]
        if len(rows) > 2 or (len(rows) == 2 and rows[1] != rows[0] + 1):
            return None
        if len(rows) == 2:
            owner[k] = rows[1]
        elif len(rows) == 1:
            owner[k] = rows[0] if k <= peak[rows[0]] else rows[0] + 1
    for p in range(n_mels + 1):
        ks = np.nonzero(owner == p)[0]
        if len(ks) and ks[-1] - ks[0] + 1 != len(ks):
            return None
    return owner


def pieces_per_segment(owner, n_mels, run=8, mirrored=False):
    """Pieces of every pair segment: a piece is the part of a segment inside one aligned run of ``run`` bins; the last bin (Nyquist) is an extra one-bin run
    (build_mel_runs layout 1 with run = 8, build_mel_pieces with run = 8 or 16).  ``mirrored``: build_mel_runs layout 0, whose upper-half runs count down from
    the Nyquist bin and whose extra bin is the middle one."""
    M = len(owner) - 1
    k = np.arange(M + 1)
    if mirrored:
        group = np.where(k < M // 2, k // run, np.where(k > M // 2, M + (M - k) // run, -1))
    else:
        group = np.where(k < M, k // run, -1)
    counts = np.zeros(n_mels + 1, int)
    for p in range(n_mels + 1):
        counts[p] = len(set(group[owner == p].tolist()))
    return counts


def expected_forms(case, power=2.0):
    """Which table forms the float32 launch of this power-of-two case can take, from the bank's data:
    ``runs`` (run-ordered, <= 16 pieces), ``many`` (eight bands per thread), ``v2`` (second-generation core), ``pieces`` (masked two-slope form, <= 15 pieces),
    ``pc`` (producer / consumer kernel), ``max_pieces`` (of the run-ordered tables that launch reads)."""
    n_fft, hop, _, n_mels, _ = case
    B = basis(case)
    M = n_fft // 2
    owner = segment_owner(B) if B.shape[1] <= 4097 else None  # (build_two_slope's packing limit: n_fft <= 8192)
    out = dict(two_slope=owner is not None, runs=False, many=False, v2=False, pieces=False, pc=False, max_pieces=0)
    if owner is None:
        return out
    many = n_fft == 512 and n_mels > 100
    v2 = hop in V2_HOPS.get(n_fft, ()) and not many
    pr = pieces_per_segment(owner, n_mels, 8, mirrored=not v2)
    out.update(many=many, v2=v2, max_pieces=int(pr.max()), runs=bool(pr.max() <= MELR_PMAX))
    p16 = pieces_per_segment(owner, n_mels, 16)
    out["pieces"] = bool(p16.max() <= MEL2_PMAX and p16.sum() <= M // 16 + n_mels + 2)
    if n_fft == 2048 and v2:
        out["pc"] = bool(power in PC_HOP_POWERS.get(hop, ()) and pr.max() <= PC_PMAX and n_mels <= PC_BANDS)
    return out


def signal_lengths(case, center=True):
    """Two clip lengths whose frame counts are 8k + 1 and 8k + 7 (the producer tile is eight frames), k >= 1."""
    n_fft, hop, _, _, _ = case
    k = 1 if n_fft >= 1024 else 2
    base = 0 if center else n_fft
    return [base + (8 * k + r - 1) * hop + hop // 3 for r in (1, 7)]


def signal(case, n, dtype=np.float32, seed=0):
    """Seeded white noise: every band of every frame is well above the rounding floor of the loudest one."""
    rng = np.random.default_rng([case[0], case[3], n, seed])
    return (0.1 * rng.standard_normal((BATCH, n))).astype(np.float32).astype(dtype)


def reference(case, y, power, dtype=np.float32, **stft_kw):
    """float64: the basis values the call uses times |STFT of the same samples in float64| ** power."""
    n_fft, hop, _, _, _ = case
    D = O.stft(np.asarray(y, dtype=np.float64), n_fft=n_fft, hop_length=hop, **stft_kw)
    return np.einsum("mf,...ft->...mt", basis(case, dtype).astype(np.float64), np.abs(D) ** power)


def worst_ratio(M, ref, B):
    """Largest |M - ref| / |ref| over the non-empty bands; the empty bands must be exactly zero and nothing NaN (asserted here: no element is exempt from both)."""
    M = np.asarray(M)
    assert M.shape == ref.shape, (M.shape, ref.shape)
    assert not np.isnan(M).any()
    empty = empty_rows(B)
    assert np.all(M[..., empty, :] == 0.0)
    r = ref[..., ~empty, :]
    assert r.min() > 0
    return float(np.max(np.abs(M[..., ~empty, :].astype(np.float64) - r) / r))


F32_BAR = 1e-4
F64_BAR = 1e-11
