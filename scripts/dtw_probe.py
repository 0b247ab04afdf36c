"""Performance probe (GPU box): device-tensor sequence.dtw, its stages, and the accumulate kernel at tile 32 and 64.

    python scripts/dtw_probe.py            # CUDA-event medians of 5 calls after a warm-up, one JSON line
    python scripts/dtw_probe.py --once     # one call of each after a warm-up (for rocprofv3 --kernel-trace --stats)
    python scripts/dtw_probe.py --small    # without the 12920 x 12920 matrix

Timed: ``dtw(X, Y)`` end to end on 12 x 1292 chroma-like features against themselves shifted by 40 frames; ``dtw(C=C)`` end to end at
1292 x 1292 and 12920 x 12920; at both sizes the stages alone through the context's calls -- cost (12 features), accumulate at tile 64 and at
tile 32, backtrack, and the widening of the step indices.  Beside the times: the launches of an accumulation (tile anti-diagonals), the
microseconds per launch, and the bytes it must move (C read, D and the uint8 step indices written, the halos read back)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from librosa_amd import _arrays  # noqa: E402
from librosa_amd import sequence as S  # noqa: E402

STEPS = np.array([[1, 1], [0, 1], [1, 0]], dtype=np.int32)
W_ADD, W_MUL = np.zeros(3), np.ones(3)


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


def stages(n, iters, gen):
    """The stages of dtw at n x n through the context's own calls, on buffers that stay allocated."""
    X = torch.rand((12, n), dtype=torch.float64, device="cuda", generator=gen)
    Y = torch.rand((12, n), dtype=torch.float64, device="cuda", generator=gen)
    C = torch.empty((n, n), dtype=torch.float64, device="cuda")
    D = torch.empty((n, n), dtype=torch.float64, device="cuda")
    idx = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    wide = torch.empty((n, n), dtype=torch.int32, device="cuda")
    path = torch.empty((2 * n - 1, 2), dtype=torch.int64, device="cuda")
    work = torch.empty(16, dtype=torch.uint8, device="cuda")
    sess = _arrays.Session(C)
    try:
        ctx = sess.ctx
        res = {"cost_ms": median_ms(lambda: ctx.dtw_cost_exec(X.data_ptr(), Y.data_ptr(), np.float64, 12, n, n, 0, C.data_ptr(), work.data_ptr()), iters)}
        res["nan_check_ms"] = median_ms(lambda: ctx.dtw_prepare_exec(C.data_ptr(), np.float64, n * n, 0, work.data_ptr()), iters)
        for tile in (64, 32):
            ms = median_ms(lambda: ctx.dtw_accumulate_exec(C.data_ptr(), n, n, STEPS, W_ADD, W_MUL, False, None, tile, D.data_ptr(), idx.data_ptr()), iters)
            launches = 2 * -(-n // tile) - 1
            res[f"accumulate_tile{tile}_ms"], res[f"accumulate_tile{tile}_launches"], res[f"accumulate_tile{tile}_us_per_launch"] = ms, launches, round(1e3 * ms / launches, 2)
        res["backtrack_ms"] = median_ms(lambda: ctx.dtw_backtrack_exec(D.data_ptr(), idx.data_ptr(), False, n, n, STEPS, False, ctx.DTW_START_END, path.data_ptr(), work.data_ptr()), iters)
        length, _ = ctx.dtw_backtrack_exec(D.data_ptr(), idx.data_ptr(), False, n, n, STEPS, False, ctx.DTW_START_END, path.data_ptr(), work.data_ptr())
        res["path_length"] = length
        res["widen_ms"] = median_ms(lambda: ctx.dtw_widen_exec(idx.data_ptr(), n * n, wide.data_ptr()), iters)
        res["accumulate_traffic_mb"] = round((8 + 8 + 1) * n * n / 1e6 + 2 * 8 * n * n / 64 / 1e6, 1)
    finally:
        sess.close()
    res["dtw_C_ms"] = median_ms(lambda: S.dtw(C=C), iters)
    return res


def main():
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 5
    gen = torch.Generator(device="cuda").manual_seed(5)
    X = torch.rand((12, 1292), dtype=torch.float32, device="cuda", generator=gen)
    X /= X.norm(dim=0, keepdim=True)
    Y = torch.roll(X, 40, dims=1) + 0.01 * torch.rand((12, 1292), dtype=torch.float32, device="cuda", generator=gen)
    if "--once" in sys.argv:
        for _ in range(2):
            S.dtw(X, Y)
            S.dtw(X, Y, subseq=True)
            torch.cuda.synchronize()
        return
    res = {"dtw_XY_1292_ms": median_ms(lambda: S.dtw(X, Y), iters), "dtw_XY_1292_subseq_ms": median_ms(lambda: S.dtw(X, Y, subseq=True), iters)}
    for n in (1292,) if "--small" in sys.argv else (1292, 12920):
        res[str(n)] = stages(n, iters, gen)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
