"""Performance probe (GPU box): device-tensor sequence.rqa, its stages, and the scoring kernel over its launch geometries.

    python scripts/rqa_probe.py            # CUDA-event medians of 5 calls after a warm-up, one JSON line
    python scripts/rqa_probe.py --once     # one call after a warm-up (for rocprofv3 --kernel-trace --stats)
    python scripts/rqa_probe.py --small    # without the 12920 x 12920 matrix

Timed at 1292 x 1292 and 12920 x 12920 on float64 sparse affinity-like input (density 0.3, weights in (0, 1]): ``rqa(sim)`` end to end at the
shipped geometry; the stages alone through the context's calls on buffers that stay allocated -- scoring at every (rows, strip) of
{8, 16, 32, 64} x {64, 128, 256, 512, 1024}, argmax, and the walk (with the length of the path it walked); and ``dtw(C=sim)`` of the same size in the same
run.  Beside the times: the launches of a scoring call, the microseconds per launch and per row, and the bytes it must move (sim read, score and
the int8 pointers written)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from librosa_amd import _arrays  # noqa: E402
from librosa_amd import sequence as S  # noqa: E402

ROWS, STRIPS = (8, 16, 32, 64), (64, 128, 256, 512, 1024)


def median_ms(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return round(float(np.median(times)), 3)


def affinity(n, gen):
    """n x n float64, density 0.3, weights in (0, 1]."""
    sim = 1.0 - torch.rand((n, n), dtype=torch.float64, device="cuda", generator=gen)
    sim *= torch.rand((n, n), dtype=torch.float64, device="cuda", generator=gen) < 0.3
    return sim


def stages(n, iters, gen):
    sim = affinity(n, gen)
    score = torch.empty((n, n), dtype=torch.float64, device="cuda")
    ptr = torch.empty((n, n), dtype=torch.int8, device="cuda")
    path = torch.empty((n, 2), dtype=torch.int64, device="cuda")
    res = {}
    sess = _arrays.Session(sim)
    try:
        ctx = sess.ctx
        work = torch.empty(ctx.RQA_WORK_BYTES, dtype=torch.uint8, device="cuda")
        table = {}
        for rows in ROWS:
            for strip in STRIPS:
                ms = median_ms(lambda: ctx.rqa_score_exec(sim.data_ptr(), np.float64, n, n, 1.0, 1.0, True, rows, strip, score.data_ptr(), ptr.data_ptr()), iters)
                launches = -(-n // rows)
                table[f"{rows}x{strip}"] = dict(ms=ms, launches=launches, us_per_launch=round(1e3 * ms / launches, 2), us_per_row=round(1e3 * ms / n, 3), workgroups=-(-n // strip))
        res["score"] = table
        best = min(table, key=lambda k: table[k]["ms"])
        res["score_best"] = best
        ctx.rqa_score_exec(sim.data_ptr(), np.float64, n, n, 1.0, 1.0, True, 0, 0, score.data_ptr(), ptr.data_ptr())
        res["argmax_ms"] = median_ms(lambda: ctx.rqa_argmax_exec(score.data_ptr(), np.float64, n * n, work.data_ptr()), iters)
        res["walk_ms"] = median_ms(lambda: ctx.rqa_backtrack_exec(ptr.data_ptr(), n, n, work.data_ptr(), path.data_ptr()), iters)
        res["path_length"] = ctx.rqa_backtrack_exec(ptr.data_ptr(), n, n, work.data_ptr(), path.data_ptr())
        res["score_traffic_mb"] = round((8 + 8 + 1) * n * n / 1e6, 1)
    finally:
        sess.close()
    res["rqa_ms"] = median_ms(lambda: S.rqa(sim), iters)
    res["rqa_score_only_ms"] = median_ms(lambda: S.rqa(sim, backtrack=False), iters)
    res["rqa_L_mode_ms"] = median_ms(lambda: S.rqa(sim, gap_onset=np.inf, gap_extend=np.inf, knight_moves=False), iters)
    del score, ptr
    res["dtw_C_ms"] = median_ms(lambda: S.dtw(C=sim), iters)
    return res


def main():
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 5
    gen = torch.Generator(device="cuda").manual_seed(5)
    if "--once" in sys.argv:
        sim = affinity(1292, gen)
        for _ in range(2):
            S.rqa(sim)
            torch.cuda.synchronize()
        return
    res = {}
    for n in (1292,) if "--small" in sys.argv else (1292, 12920):
        res[str(n)] = stages(n, iters, gen)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
