#!/usr/bin/env python3
"""Development aid: static instruction budget of the producer / consumer mel kernel's consumer wave (lra_kernels_pc.h).

Cross-compiles instantiation group 11 (lra_inst.hip) for gfx950, cuts out one stft_pc_kernel instance (default: the bench's,
FftCfg<10,4,float,64,2,1,0,0>, hop n_fft / 4, |X|^2) and finds the consumer's frame loop(s): the depth-1 loops that hold both of the
consumer's priorities (s_setprio kPcPrioCA = 0, kPcPrioCB = 1).  Every basic block of such a loop is counted (VALU, SALU, LDS,
VMEM) and classed:
  wait   the bounded sleeping poll (s_sleep) and the sticky-flag report -- not run while the ready flag is already set
  burst  blocks that store to the output (global_store) -- a whole tile once per eight frames and band, partial tiles at slot ends
  hot    everything else: run once per served frame (two serves per loop trip, one per producer slot)
and the summary prints hot instructions per served frame and the full-burst blocks amortised over eight frames.

  python scripts/pc_consumer_isa.py [--asm FILE] [--kernel REGEX] [--blocks]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_KERNEL = r"_Z14stft_pc_kernelIN3lra6FftCfgILi10ELi4EfLi64ELi2ELb1ELb0ELi0EEELi4ELi2EE"


def compile_group(out):
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-DLRA_INST_GROUP=11", "-S", "--cuda-device-only",
           "-o", out, os.path.join(ROOT, "librosa_amd", "csrc", "lra_inst.hip")]
    subprocess.run(cmd, check=True, cwd=os.path.join(ROOT, "librosa_amd", "csrc"))


def cut_kernel(text, pat):
    lines = text.splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(pat + r".*:", l) and not l.startswith("\t"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    return lines[start:end + 1]


def classify(ins):
    op = ins.split()[0]
    if op.startswith(("v_readfirstlane", "v_readlane", "v_writelane")):
        return "valu"
    if op.startswith("v_"):
        return "valu"
    if op.startswith(("ds_",)):
        return "lds"
    if op.startswith(("global_", "buffer_", "scratch_", "flat_")):
        return "vmem"
    if op.startswith("s_") and not op.startswith(("s_nop", "s_waitcnt", "s_setprio", "s_sleep", "s_barrier", "s_endpgm")):
        return "salu"
    return None


def blocks_of(lines):
    """[(label, header comment, [instructions])] in program order."""
    out, cur = [], None
    for l in lines:
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", l) or re.match(r"^; (%bb\.\d+):(.*)$", l)
        if m:
            cur = [m.group(1), m.group(2), []]
            out.append(cur)
            continue
        s = l.split(";")[0].strip()
        if cur is None or not s or s.startswith(".") or s.endswith(":"):
            continue
        cur[2].append(s)
    return out


def consumer_loops(blocks):
    """Depth-1 loop headers whose loops hold s_setprio 0 and s_setprio 1 -> list of (header, [block indices])."""
    loops = {}
    for i, (lab, hdr, ins) in enumerate(blocks):
        m = re.search(r"Loop: Header=BB(\d+_\d+) Depth=1", hdr) or re.search(r"Parent Loop BB(\d+_\d+) Depth=1", hdr)
        if "=>This Loop Header: Depth=1" in hdr:
            loops.setdefault(lab.lstrip(".LBB"), []).append(i)
        elif m:
            loops.setdefault(m.group(1), []).append(i)
    found = []
    for h, idx in loops.items():
        ops = [x for i in idx for x in blocks[i][2]]
        if "s_setprio 0" in ops and "s_setprio 1" in ops:
            found.append((h, idx))
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", help="an existing group-11 assembly file (default: compile one)")
    ap.add_argument("--kernel", default=DEFAULT_KERNEL, help="mangled-name prefix of the instance")
    ap.add_argument("--blocks", action="store_true", help="print every block of the loop(s)")
    o = ap.parse_args()
    if o.asm:
        text = open(o.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            f = os.path.join(d, "g11.s")
            compile_group(f)
            text = open(f).read()
    blocks = blocks_of(cut_kernel(text, o.kernel))
    loops = consumer_loops(blocks)
    if not loops:
        sys.exit("no consumer loop found")
    print(f"kernel {o.kernel}")
    for h, idx in loops:
        uniform = any(x.startswith("s_set_gpr_idx_on") for i in idx for x in blocks[i][2])
        tot = {c: {"valu": 0, "salu": 0, "lds": 0, "vmem": 0} for c in ("hot", "burst", "wait")}
        full = {"valu": 0, "salu": 0, "lds": 0, "vmem": 0}
        if o.blocks:
            print(f"\nloop BB{h} ({'uniform tile slot' if uniform else 'per-lane tile slot'}): block  class  VALU SALU LDS VMEM")
        for i in idx:
            lab, _, ins = blocks[i]
            cnt = {"valu": 0, "salu": 0, "lds": 0, "vmem": 0}
            for x in ins:
                c = classify(x)
                if c:
                    cnt[c] += 1
            cls = "wait" if any(x.startswith(("s_sleep", "global_atomic", "v_mbcnt")) for x in ins) else \
                  "burst" if any(x.startswith("global_store") for x in ins) else "hot"
            for k in cnt:
                tot[cls][k] += cnt[k]
            if cls == "burst" and any(x.startswith("global_store_dwordx4") for x in ins):
                for k in cnt:
                    full[k] += cnt[k]
            if o.blocks:
                print(f"  {lab:12s} {cls:5s} {cnt['valu']:4d} {cnt['salu']:4d} {cnt['lds']:3d} {cnt['vmem']:4d}")
        serves = 2  # one serve per producer slot per loop trip
        print(f"\nconsumer loop BB{h} ({'uniform tile slot: n_frames % 4 == 0' if uniform else 'per-lane tile slot'})")
        for c in ("hot", "burst", "wait"):
            t = tot[c]
            print(f"  {c:5s} blocks, whole loop trip: VALU {t['valu']:4d}  SALU {t['salu']:4d}  LDS {t['lds']:3d}  VMEM {t['vmem']:3d}")
        hv = tot["hot"]
        print(f"  per served frame: hot VALU {hv['valu'] / serves:.1f}  SALU {hv['salu'] / serves:.1f}  LDS {hv['lds'] / serves:.1f}"
              f"  + full bursts amortised over 8 frames: VALU {full['valu'] / serves / 8:.1f}  SALU {full['salu'] / serves / 8:.1f}")


if __name__ == "__main__":
    main()
