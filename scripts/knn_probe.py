"""Performance probe (GPU box): device-tensor segment.recurrence_matrix, the selection kernel over its launch geometries, and the baseline the
parent commit lets a user run on the device.

    python scripts/knn_probe.py            # CUDA-event medians of 5 calls after a warm-up, one JSON line
    python scripts/knn_probe.py --once     # one call after a warm-up (for rocprofv3 --kernel-trace --stats)
    python scripts/knn_probe.py --small    # t = 1292 only

Timed at t = 1292, 5168 and 12920 frames of d = 12 and d = 84 float32 features, the default ``k = 2 ceil(sqrt(t - 2 width + 1))``, ``width = 3``:
``recurrence_matrix(x, width=3, mode="affinity")`` end to end, sparse and dense; ``lra_knn_select_exec`` alone (selection and the sort of the rows)
on buffers that stay allocated, at every (rows, tile) of {4, 8, 16} x {64, 128, 256, 512} that is served; and the baseline in the same run:
``lra_dtw_cost_exec`` into a t x t float64 matrix, then ``torch.topk`` of ``k + 2 width`` per row.  Beside the times: the bytes of the lists against
the bytes of the matrix."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from librosa_amd import _arrays, _native  # noqa: E402
from librosa_amd import segment as G  # noqa: E402

ROWS, TILES = (4, 8, 16), (64, 128, 256, 512)
WIDTH = 3


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


def stages(t, d, iters, gen):
    x = torch.randn((d, t), dtype=torch.float32, device="cuda", generator=gen)
    k = int(2 * np.ceil(np.sqrt(t - 2 * WIDTH + 1)))
    res = dict(k=k, list_mb=round(t * k * 12 / 1e6, 2), matrix_mb=round(8 * t * t / 1e6, 1))
    lib = _native.load_library()
    cnt = torch.empty(t, dtype=torch.int32, device="cuda")
    idx = torch.empty((t, k), dtype=torch.int32, device="cuda")
    dist = torch.empty((t, k), dtype=torch.float64, device="cuda")
    sess = _arrays.Session(x)
    try:
        ctx = sess.ctx
        table = {}
        for rows in ROWS:
            for tile in TILES:
                if not lib.lra_knn_lds_bytes(rows, tile, k):
                    continue
                table[f"{rows}x{tile}"] = median_ms(lambda: ctx.knn_select_exec(x.data_ptr(), x.data_ptr(), np.float32, d, t, t, 0, k, WIDTH, True, rows, tile, cnt.data_ptr(), idx.data_ptr(),
                                                                                dist.data_ptr()), iters)
        res["select"] = table
        res["select_best"] = min(table, key=table.get)
        res["select_shipped_ms"] = median_ms(lambda: ctx.knn_select_exec(x.data_ptr(), x.data_ptr(), np.float32, d, t, t, 0, k, WIDTH, True, 0, 0, cnt.data_ptr(), idx.data_ptr(), dist.data_ptr()),
                                             iters)
        # the baseline: the whole cost matrix, then the k + 2 width smallest of every row
        C = torch.empty((t, t), dtype=torch.float64, device="cuda")
        work = torch.empty(16, dtype=torch.uint8, device="cuda")
        res["baseline_cost_ms"] = median_ms(lambda: ctx.lib.lra_dtw_cost_exec(ctx.handle, x.data_ptr(), x.data_ptr(), _native.dtype_code(np.float32), d, t, t, 0, C.data_ptr(), work.data_ptr(), None),
                                            iters)
        res["baseline_topk_ms"] = median_ms(lambda: torch.topk(C, k + 2 * WIDTH, dim=1, largest=False), iters)
        res["baseline_ms"] = round(res["baseline_cost_ms"] + res["baseline_topk_ms"], 3)
        del C
    finally:
        sess.close()
    res["recurrence_sparse_ms"] = median_ms(lambda: G.recurrence_matrix(x, width=WIDTH, mode="affinity", sparse=True), iters)
    res["recurrence_dense_ms"] = median_ms(lambda: G.recurrence_matrix(x, width=WIDTH, mode="affinity"), iters)
    res["recurrence_connectivity_sym_ms"] = median_ms(lambda: G.recurrence_matrix(x, width=WIDTH, sym=True, sparse=True), iters)
    return res


def main():
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 5
    gen = torch.Generator(device="cuda").manual_seed(5)
    if "--once" in sys.argv:
        x = torch.randn((12, 1292), dtype=torch.float32, device="cuda", generator=gen)
        for _ in range(2):
            G.recurrence_matrix(x, width=WIDTH, mode="affinity", sparse=True)
            torch.cuda.synchronize()
        return
    res = {}
    for t in (1292,) if "--small" in sys.argv else (1292, 5168, 12920):
        for d in (12, 84):
            res[f"{t}x{d}"] = stages(t, d, iters, gen)
            print(json.dumps({f"{t}x{d}": res[f"{t}x{d}"]}), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
