"""Development aid: LDS-array cycles and bank-conflict cycles per frame of the fused mel kernel (n_fft = 2048, one wave64 per frame), from the
kernel's own address formulas and the banking rules of gfx950's LDS (GROUPS below: the lane groups one LDS cycle serves and the banks they are
spread over, per instruction).  Used to choose layouts offline; the counters (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE, profiles/) are what decides.

The model follows the kernel as it is:
  * the two FFT exchanges in the layouts of csrc/lra_fft.h ("exchange addresses"): --layout split (pass 0 -> 1 transposed with row pitch 66,
    pass 1 -> last unpadded: FftCfg::X1T / X2U) or --layout phys (every element i at i + (i >> padshift): the layout of every other
    configuration, and of these cores before profiles/r09_lds_layout_ab.md); the radix 16-16-4 core's exchange 1 is listed beside it;
  * the swizzled power row (v2_pw_index: runs of 8 bins, the two 16-byte halves swapped where bit 7 of the bin is set), written with
    ds_write_b32 in butterfly order and read back as ds_read_b128 runs;
  * the running sums (pitch mel_runs_pitch = TF + kMelRsPitchExtra pairs) and the band gather as ds_read_b64 PAIR reads (pc_pair_ld);
  * both forms: --form pc (producer / consumer, lra_kernels_pc.h: weights in the consumer's registers, the zero slot written once per
    workgroup) and --form one (stft2_kernel<OUT_MELR>: weights read from the shared table, the zero slot written every frame).

    python scripts/lds_model.py [--layout split|phys] [--form pc|one] [--padshift 4] [--rs-extra 0] [--sites]
    python scripts/lds_model.py --sweep-pitch        # gather conflicts per running-sum pitch over the n_fft = 2048 banks of tests/mel_bank_cases.py
"""
import argparse
import collections
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

GROUPS = {
    "read_b32": ([list(range(0, 32)), list(range(32, 64))], 32),
    "read_b64": ([list(range(0, 32)), list(range(32, 64))], 64),
    "read_b128": ([[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
                   [32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59], [36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63]], 64),
    "write_b32": ([list(range(0, 32)), list(range(32, 64))], 32),
    "write_b64": ([list(range(16 * g, 16 * g + 16)) for g in range(4)], 32),
}
WIDTH = {"read_b32": 4, "read_b64": 8, "read_b128": 16, "write_b32": 4, "write_b64": 8}
M, TF, R = 1024, 64, 16
X1_PITCH = 66  # FftCfg::X1_PITCH


def cycles(kind, addrs, active=None):
    """(array cycles, conflict cycles) of one wave-instruction; addrs[lane] = byte address (None / inactive lanes skipped)."""
    groups, nb = GROUPS[kind]
    total = conf = 0
    for g in groups:
        per_bank = collections.defaultdict(set)
        for l in g:
            if addrs[l] is None or (active is not None and not active[l]):
                continue
            for d in range(WIDTH[kind] // 4):
                a = addrs[l] + 4 * d
                per_bank[(a // 4) % nb].add(a // 4)
        worst = max((len(v) for v in per_bank.values()), default=1)
        total += max(1, worst)
        conf += max(0, worst - 1)
    return total, conf


def pw_index(k):
    """v2_pw_index, swizzled form (lra_kernels2.h)."""
    return (k >> 3) * 8 + ((((k >> 2) ^ (k >> 7)) & 1) << 2) + (k & 3)


def default_bank(n_mels=128):
    import librosa_amd.filters as F

    return F.mel(sr=22050, n_fft=2048, n_mels=n_mels).astype(np.float32)


def bank_pieces(B, rs_pitch):
    """Piece totals (byte addresses of (A, B) pairs in the running-sum area) each band's two lists gather, as lra_mel.h lays them out for the
    run-ordered form: thread t's runs are bins 8 t + j and M/2 + 8 t + j, a piece ends where the owning pair segment changes."""
    n_bins = B.shape[1]
    owner = np.full(n_bins, -1)
    peak = B.argmax(axis=1)
    for k in range(n_bins):
        nz = np.nonzero(B[:, k])[0]
        if len(nz) == 2:
            owner[k] = nz[1]
        elif len(nz) == 1:
            owner[k] = nz[0] if k <= peak[nz[0]] else nz[0] + 1
    half, bpl = M // 2, 8
    bin_of = lambda t, jj: bpl * t + jj if jj < bpl else half + bpl * t + (jj - bpl)
    pieces = collections.defaultdict(list)
    for t in range(TF):
        for run in range(2):
            cur = -2
            for j in range(bpl):
                jj = run * bpl + j
                seg = owner[bin_of(t, jj)]
                restart = j == 0 or (seg >= 0 and cur >= 0 and seg != cur)
                if restart:
                    if j > 0 and cur >= 0:
                        pieces[cur].append(((jj - 1) * rs_pitch + t) * 8)
                    cur = seg if seg >= 0 else -2
                elif seg >= 0 and cur < 0:
                    cur = seg
            if cur >= 0:
                pieces[cur].append(((run * bpl + bpl - 1) * rs_pitch + t) * 8)
    zero = 16 * rs_pitch * 8
    mid = zero + 8
    if owner[M] >= 0:
        pieces[owner[M]].append(mid)
    return pieces, max((len(v) for v in pieces.values()), default=0), zero, mid


def gather_rows(B, rs_extra, add):
    """The band gather: sixteen ds_read_b64 pair reads per frame (bands 2 tf, 2 tf + 1; the B list of band m holds segment m's pieces, the A list
    segment m + 1's; absent pieces and lanes without a band address the zero pair)."""
    n_mels = B.shape[0]
    pieces, pmax_bank, zero, mid = bank_pieces(B, TF + rs_extra)
    pmax = max(4, pmax_bank)
    for b in range(2):
        for e in range(2 * pmax):
            def fn(tf, b=b, e=e):
                m = 2 * tf + b
                if m >= n_mels:
                    return zero
                lst = pieces.get(m if e < pmax else m + 1, [])
                q = e % pmax
                return lst[q] if q < len(lst) else zero
            add(f"combine band {b} entry {e}", "read_b64", fn)
    return pmax_bank, zero, mid


def model(layout="split", form="pc", padshift=4, rs_extra=0, w_pad=2, B=None, verbose=True, sites=False):
    phys = lambda i: i + (i >> padshift)
    pstride = lambda c: c + (c >> padshift)
    rows = []

    def add(name, kind, fn, active=None):
        t, c = cycles(kind, [fn(l) for l in range(64)], active)
        rows.append((name, kind, t, c))

    mirror = lambda tf: 64 if tf == 0 else 128 - tf
    if layout == "split":
        # exchange 1, transposed: output j of lane tf at unit tf + 66 j; pass-1 lane l reads unit 66 (l & 15) + (l >> 4) + (i TF + j sin) / 16
        for j in range(16):
            add(f"pass0 write j={j}", "write_b64", lambda tf, j=j: (tf + X1_PITCH * j) * 8)
        for i in range(2):
            for j in range(8):
                add(f"pass1 read i={i} j={j}", "read_b64", lambda tf, i=i, j=j: (X1_PITCH * (tf & 15) + (tf >> 4) + ((i * 64 + j * 128) >> 4)) * 8)
        # exchange 2, unpadded
        for i in range(2):
            for j in range(8):
                add(f"pass1 write i={i} j={j}", "write_b64", lambda tf, i=i, j=j: ((((tf - (tf & 15)) << 3) + (tf & 15)) + i * 512 + j * 16) * 8)
        for j in range(8):
            add(f"last read A j={j}", "read_b64", lambda tf, j=j: (tf + j * 128) * 8)
            add(f"last read B j={j}", "read_b64", lambda tf, j=j: (mirror(tf) + j * 128) * 8)
        x1_read_1664 = lambda tf, j: (X1_PITCH * (tf & 15) + (tf >> 4) + ((j * 64) >> 4)) * 8
    else:
        # pass 0 write: (tf (r + 1) + j) 8, r = 2^padshift ... only for padshift == logr(0) == 4 is this the layout; general: phys(tf 16 + j)
        for j in range(16):
            add(f"pass0 write j={j}", "write_b64", lambda tf, j=j: phys(tf * 16 + j) * 8)
        for i in range(2):
            for j in range(8):
                add(f"pass1 read i={i} j={j}", "read_b64", lambda tf, i=i, j=j: (phys(tf) + i * pstride(64) + j * pstride(128)) * 8)
        for i in range(2):
            for j in range(8):
                add(f"pass1 write i={i} j={j}", "write_b64", lambda tf, i=i, j=j: (phys(((tf - (tf & 15)) << 3) + (tf & 15)) + i * pstride(512) + j * pstride(16)) * 8)
        for j in range(8):
            add(f"last read A j={j}", "read_b64", lambda tf, j=j: (phys(tf) + j * pstride(128)) * 8)
            add(f"last read B j={j}", "read_b64", lambda tf, j=j: (phys(mirror(tf)) + j * pstride(128)) * 8)
        x1_read_1664 = lambda tf, j: (phys(tf) + j * pstride(64)) * 8
    n_core = len(rows)
    # power row (swizzled): pair slot q of lane tf holds bins k = tf + q s and M - k (lane 0, q >= r/2: k = s/2 + (q - r/2) s); bin M/2 by lane 0
    tfh = lambda tf: 64 * (1 - 8) if tf == 0 else tf
    for q in range(8):
        add(f"power write k q={q}", "write_b32", lambda tf, q=q: pw_index((tf if q < 4 else tfh(tf)) + q * 128) * 4)
        add(f"power write M-k q={q}", "write_b32", lambda tf, q=q: pw_index(M - ((tf if q < 4 else tfh(tf)) + q * 128)) * 4)
    add("power write mid", "write_b32", lambda tf: pw_index(M // 2) * 4, active=[l == 0 for l in range(64)])
    for run in range(2):
        for h in range(2):
            add(f"runs read run={run} h={h}", "read_b128", lambda tf, run=run, h=h: pw_index(8 * (run * TF + tf) + 4 * h) * 4)
    add("runs read extra", "read_b32", lambda tf: pw_index(M) * 4 if tf == 0 else 0)
    if form == "one":
        SH = 1 << 20  # the shared table lives elsewhere; only its bank matters
        for run in range(2):
            for j in range(0, 8, 2):
                add(f"weights read run={run} j={j}", "read_b128", lambda tf, run=run, j=j: SH + ((8 + w_pad) * (run * TF + tf) + j) * 8)
    rs_pitch = TF + rs_extra
    for jj in range(16):
        add(f"sums write jj={jj}", "write_b64", lambda tf, jj=jj: (jj * rs_pitch + tf) * 8)
    if B is None:
        B = default_bank()
    lane0 = [l == 0 for l in range(64)]
    pmax, zero, mid = gather_rows(B, rs_extra, add)
    add("sums write mid", "write_b64", lambda tf: mid, active=lane0)
    if form == "one":
        add("sums write zero", "write_b64", lambda tf: zero, active=lane0)  # (pc: once per workgroup, pc_consumer_prologue)
    tot = sum(r[2] for r in rows)
    con = sum(r[3] for r in rows)
    if verbose:
        grp = collections.OrderedDict()
        for name, kind, t, c in rows:
            key = name.split(" ")[0] + " " + name.split(" ")[1] + " (" + kind + ")"
            g = grp.setdefault(key, [0, 0, 0])
            g[0] += 1; g[1] += t; g[2] += c
        for k, (n, t, c) in grp.items():
            print(f"{k:34s} n={n:3d} cycles={t:4d} conflict={c:4d}")
        if sites:
            for name, kind, t, c in rows[:n_core]:
                print(f"    {name:28s} {kind:10s} cycles={t} conflict={c}")
        print(f"layout {layout}, form {form}: total {tot} cycles per frame, {con} conflict cycles ({con / tot:.1%}); pmax {pmax}")
        # the radix 16-16-4 core's exchange 1 (its middle pass: one radix-16 butterfly per lane, inputs 64 elements apart)
        t16 = c16 = 0
        for j in range(16):
            t, c = cycles("read_b64", [x1_read_1664(l, j) for l in range(64)])
            t16 += t; c16 += c
        print(f"radix 16-16-4, pass1 read (read_b64)  n= 16 cycles={t16:4d} conflict={c16:4d}")
    return tot, con


def sweep_pitch(extras=(0, 1, 2, 3, 4)):
    """Gather cycles / conflicts of the sixteen pair reads per running-sum pitch TF + extra, for every n_fft = 2048 bank of tests/mel_bank_cases.py
    the run-ordered form serves (<= 16 pieces; the producer / consumer kernel takes those with <= 4 pieces and <= 128 bands).  extra <= 4 keeps the
    running sums inside the one-wave kernel's frame area (stft_block2's static_assert) and PcLayout::BYTES at 33.9 + 0.125 extra KB <= 40 KB."""
    import mel_bank_cases as MB

    seen = set()
    print(f"{'bank':42s} pmax " + " ".join(f"+{e}: cyc/conf" for e in extras))
    for case in MB.CASES:
        n_fft, _, sr, n_mels, kw = case
        key = (sr, n_mels, tuple(sorted((k, str(v)) for k, v in kw.items())))
        if n_fft != 2048 or key in seen:
            continue
        seen.add(key)
        B = MB.basis(case)
        cells, pmax = [], 0
        for e in extras:
            rows = []
            pmax, _, _ = gather_rows(B, e, lambda name, kind, fn: rows.append(cycles(kind, [fn(l) for l in range(64)])))
            cells.append(f"{sum(r[0] for r in rows):4d}/{sum(r[1] for r in rows):3d}")
        if pmax > 16:
            continue
        tag = MB.case_id(case)[len("2048-") :].split("-", 1)[1] + (" (pc)" if pmax <= 4 and n_mels <= 128 else "")
        print(f"{tag:42s} {pmax:4d} " + "   ".join(cells))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", choices=("split", "phys"), default="split")
    ap.add_argument("--form", choices=("pc", "one"), default="pc")
    ap.add_argument("--padshift", type=int, default=4, help="--layout phys only")
    ap.add_argument("--rs-extra", type=int, default=0, help="kMelRsPitchExtra")
    ap.add_argument("--w-pad", type=int, default=2)
    ap.add_argument("--sites", action="store_true", help="list the exchanges' wave instructions one by one")
    ap.add_argument("--sweep-pitch", action="store_true")
    a = ap.parse_args()
    if a.sweep_pitch:
        sweep_pitch()
    else:
        model(a.layout, a.form, a.padshift, a.rs_extra, a.w_pad, sites=a.sites)
