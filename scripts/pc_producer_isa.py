#!/usr/bin/env python3
"""Development aid: static instruction budget of the producer / consumer mel kernel's producer wave (lra_kernels_pc.h).

Sibling of pc_consumer_isa.py (same block parser, same instruction classes).  Cross-compiles instantiation group 11 (lra_inst.hip) for
gfx950, cuts out one stft_pc_kernel instance (default: the bench's, FftCfg<10,4,float,64,2,1,0,0>, hop n_fft / 4, |X|^2) and finds the
producer's frame loop: the depth-1 loop that holds both of the producer's priorities (s_setprio kPcPrioPA = 3, kPcPrioPS = 2).
Every basic block of the loop is counted (VALU, SALU, LDS, VMEM; VALU split into packed v_pk_*, other arithmetic and the rest: moves,
selects, shifts, integer and address work) and classed:
  wait    the bounded sleeping poll on consumed[s] (s_sleep) and the sticky-flag report -- not run while the consumer keeps up
  edge    the clip-edge sample loads: the unaligned arm and the np.pad index fold (4-byte global loads and the blocks between them)
  window  the block that holds the rotation switches (v2_window_rotating): one arm of four runs per residue class, so its run count is
          walked per rotation (the slot's first frame apart) and printed next to the static one
  hot     everything else: the straight-line path of every frame
Blocks are printed in program order; the summary adds the hot blocks and the window block's run count.

  python scripts/pc_producer_isa.py [--asm FILE] [--kernel REGEX] [--blocks]
"""
import argparse
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pc_consumer_isa import DEFAULT_KERNEL, classify, compile_group, cut_kernel  # noqa: E402

ARITH = ("v_add_f", "v_sub_f", "v_mul_f", "v_fma_f", "v_fmac_f", "v_mac_f", "v_mad_f", "v_sqrt_f", "v_rsq_f", "v_rcp_f", "v_max_f", "v_min_f",
         "v_ldexp_f", "v_frexp", "v_exp_f", "v_log_f", "v_div_f", "v_trunc_f", "v_rndne_f", "v_floor_f", "v_fract_f", "v_cmp_class", "v_cmp_o_f",
         "v_cmp_u_f", "v_cmp_lt_f", "v_cmp_gt_f", "v_cmp_le_f", "v_cmp_ge_f", "v_cmp_eq_f", "v_cmp_neq_f", "v_cmp_nlt_f", "v_cmp_ngt_f",
         "v_cmp_nle_f", "v_cmp_nge_f", "v_cmp_lg_f", "v_cmp_nlg_f", "v_cvt_")
KEYS = ("valu", "pk", "arith", "rest", "salu", "lds", "vmem")


def count(ins_list):
    c = dict.fromkeys(KEYS, 0)
    for x in ins_list:
        k = classify(x)
        if not k:
            continue
        c[k] += 1
        if k == "valu":
            op = x.split()[0]
            c["pk" if op.startswith("v_pk_") else "arith" if op.startswith(ARITH) else "rest"] += 1
    return c


def blocks_with_labels(lines):
    """As pc_consumer_isa.blocks_of, but keeps the asm-local labels of the rotation switch (.Lrot*) as pseudo-instructions."""
    out, cur = [], None
    for l in lines:
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", l) or re.match(r"^; (%bb\.\d+):(.*)$", l)
        if m:
            cur = [m.group(1), m.group(2), []]
            out.append(cur)
            continue
        s = l.split(";")[0].strip()
        if cur is None or not s:
            continue
        if re.match(r"^\.Lrot\w+:$", s):
            cur[2].append(s)
            continue
        if s.startswith(".") or s.endswith(":"):
            continue
        cur[2].append(s)
    return out


def walk_rotation(ins, rot):
    """Instructions of a window block that run for rotation `rot` (not the slot's first frame): follows the scalar ladders of the
    rotation switches.  Each switch compares one SGPR (the rotation) with s_cmp_lg_u32 and another (the frame counter) with s_cmp_eq_u32."""
    labels = {x[:-1]: i for i, x in enumerate(ins) if x.startswith(".Lrot")}
    run, i, scc, taken = [], 0, False, 0
    while i < len(ins):
        x = ins[i]
        if x.startswith(".Lrot"):
            i += 1
            continue
        run.append(x)
        op = x.split()[0]
        arg = x[len(op):].split(",")
        tgt = arg[0].strip()
        if op == "s_cmp_lg_u32" and tgt_is_rot(ins, i):
            scc = rot != int(arg[1])
        elif op == "s_cmp_eq_u32" and tgt_is_rot(ins, i):
            scc = False  # frame counter == 0: the slot's first frame only
        elif op == "s_cbranch_scc1" and tgt in labels:
            if scc:
                i = labels[tgt]
                taken += 1
                continue
        elif op == "s_branch" and tgt in labels:
            i = labels[tgt]
            taken += 1
            continue
        i += 1
    return run, taken


def tgt_is_rot(ins, i):
    """True when the compare at i feeds a branch to a rotation-switch label."""
    return i + 1 < len(ins) and ins[i + 1].split()[0] == "s_cbranch_scc1" and ins[i + 1].split()[1].startswith(".Lrot")


def producer_loop(blocks):
    loops = {}
    for i, (lab, hdr, _) in enumerate(blocks):
        m = re.search(r"Loop: Header=BB(\d+_\d+) Depth=1", hdr) or re.search(r"Parent Loop BB(\d+_\d+) Depth=1", hdr)
        if "=>This Loop Header: Depth=1" in hdr:
            loops.setdefault(lab.lstrip(".LBB"), []).append(i)
        elif m:
            loops.setdefault(m.group(1), []).append(i)
    for h, idx in loops.items():
        ops = [x for i in idx for x in blocks[i][2]]
        if "s_setprio 3" in ops and "s_setprio 2" in ops:
            return h, sorted(idx)
    return None, []


def classes(blocks, idx):
    """block index -> class.  hipcc lays the cold sample-load arms (the unaligned arm and the np.pad index fold with its 4-byte loads) out
    behind the frame's body: the edge path is every block of the loop behind the last block that touches the LDS or belongs to the poll,
    as long as that tail holds the 4-byte loads."""
    cls = {}
    is_wait = lambda ins: any(x.startswith(("s_sleep", "global_atomic", "v_mbcnt")) for x in ins)
    body_end = max(i for i in idx if is_wait(blocks[i][2]) or any(x.startswith("ds_") for x in blocks[i][2]))
    tail = [i for i in idx if i > body_end]
    if not any(re.match(r"global_load_dword\s", x) for i in tail for x in blocks[i][2]):
        tail = []
    for i in idx:
        ins = blocks[i][2]
        if is_wait(ins):
            cls[i] = "wait"
        elif any(x.startswith(".Lrot") for x in ins):
            cls[i] = "window"
        elif i in tail:
            cls[i] = "edge"
        else:
            cls[i] = "hot"
    return cls


def fmt(c):
    return (f"VALU {c['valu']:4d} (pk {c['pk']:3d}  arith {c['arith']:3d}  rest {c['rest']:3d})  SALU {c['salu']:3d}  LDS {c['lds']:3d}  VMEM {c['vmem']:2d}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", help="an existing group-11 assembly file (default: compile one)")
    ap.add_argument("--kernel", default=DEFAULT_KERNEL, help="mangled-name prefix of the instance")
    ap.add_argument("--blocks", action="store_true", help="print the small blocks too (default: blocks of ten or more instructions)")
    o = ap.parse_args()
    if o.asm:
        text = open(o.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            f = os.path.join(d, "g11.s")
            compile_group(f)
            text = open(f).read()
    blocks = blocks_with_labels(cut_kernel(text, o.kernel))
    h, idx = producer_loop(blocks)
    if h is None:
        sys.exit("no producer loop found")
    cls = classes(blocks, idx)
    print(f"kernel {o.kernel}")
    print(f"producer loop BB{h}: {len(idx)} blocks")
    tot = {c: dict.fromkeys(KEYS, 0) for c in ("hot", "window", "edge", "wait")}
    win_run, win_taken = dict.fromkeys(KEYS, 0), 0
    for i in idx:
        lab, _, ins = blocks[i]
        real = [x for x in ins if not x.startswith(".Lrot")]
        c = count(real)
        for k in KEYS:
            tot[cls[i]][k] += c[k]
        note = ""
        if cls[i] == "window":
            per_rot = [walk_rotation(ins, r) for r in range(4)]
            runs = [count(r) for r, _ in per_rot]
            for k in KEYS:
                win_run[k] += round(sum(r[k] for r in runs) / 4)
            win_taken += round(sum(t for _, t in per_rot) / 4)
            note = f"   run per frame: VALU {round(sum(r['valu'] for r in runs) / 4)}  SALU {round(sum(r['salu'] for r in runs) / 4)}"
        prio = [x for x in real if x.startswith("s_setprio")]
        if o.blocks or sum(c[k] for k in ("valu", "salu", "lds", "vmem")) >= 10:
            print(f"  {lab:10s} {cls[i]:6s} {fmt(c)}  {' '.join(prio)}{note}")
    print()
    for c in ("hot", "window", "edge", "wait"):
        print(f"  {c:6s} blocks, static: {fmt(tot[c])}")
    print(f"  window block as run (one arm of four per residue class, mean over the rotations): {fmt(win_run)}  taken branches {win_taken}")
    per = {k: tot["hot"][k] + win_run[k] for k in KEYS}
    print(f"  per frame, hot + window as run: {fmt(per)}")
    print(f"  of the VALU per frame: packed {per['pk']}, other arithmetic {per['arith']}, not arithmetic {per['rest']}")


if __name__ == "__main__":
    main()
