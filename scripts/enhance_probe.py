"""Performance probe (GPU box): device-tensor segment.path_enhance over its tiles, recurrence_to_lag and feature.stack_memory against a device
copy of their own traffic, and the scipy.ndimage route on the same host.

    python scripts/enhance_probe.py            # CUDA-event medians of 5 calls after a warm-up, one JSON line per stage
    python scripts/enhance_probe.py --once     # one call after a warm-up (for rocprofv3 --kernel-trace --stats)
    python scripts/enhance_probe.py --small    # 1292 x 1292 only

Timed: ``path_enhance(R, 51, window="hann", n_filters=7)`` end to end on 1292 x 1292 and 12920 x 12920 random matrices, float64 and float32, at
the library's tile and at every tile of ``TILES`` in alternating rounds of one process; beside the times the counts the kernel's work follows
from -- taps, LDS bytes read (8 per tap and cell), float64 operations (a product and a sum per tap and cell), HBM bytes (matrix in, matrix out) --
and the least time each implies (LDS at the 256 B/clk/CU of ``ds_read_b64``, float64 at 64 lanes/clk/CU, both at 256 CUs and 2.4 GHz; HBM at the
rate of the device copy measured in the same run).  ``recurrence_to_lag(pad=True)`` on the same matrices and ``stack_memory(n_steps=10, delay=3)``
on 12 x 4 000 000 float32 features as bytes moved per second, against ``Tensor.copy_`` of a buffer of the same traffic.  The baseline: the
``n_filters`` calls of ``scipy.ndimage.convolve`` and their maximum on 1292 x 1292 float64, once, on this host."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from librosa_amd import feature as F  # noqa: E402
from librosa_amd import filters  # noqa: E402
from librosa_amd import segment as G  # noqa: E402

TILES = ((64, 64), (32, 64), (16, 64), (32, 32), (16, 32), (16, 16))
N, N_FILTERS = 51, 7
CUS, GHZ = 256, 2.4


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return round(float(np.median([timed_ms(fn) for _ in range(iters)])), 3)


def at_tile(tile, fn):
    saved = G.ENHANCE_ROWS, G.ENHANCE_COLS
    G.ENHANCE_ROWS, G.ENHANCE_COLS = tile
    try:
        return fn()
    finally:
        G.ENHANCE_ROWS, G.ENHANCE_COLS = saved


def copy_gbps(nbytes, iters):
    """The device copy of a buffer whose read plus write traffic is ``nbytes``."""
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty_like(src)
    ms = median_ms(lambda: dst.copy_(src), iters)
    return round(nbytes / ms / 1e6, 1)


def enhance(side, dtype, iters, gen, tiles):
    R = torch.rand((side, side), dtype=dtype, device="cuda", generator=gen)
    taps, _ = G._filter_taps([filters.diagonal_filter_cached("hann", N, slope=r) for r in np.logspace(-1, 1, num=N_FILTERS, base=2)])
    cells, esize = side * side, R.element_size()
    res = dict(taps=int(taps.size), cells=cells, lds_read_gb=round(8 * taps.size * cells / 1e9, 2), fp64_gop=round(2 * taps.size * cells / 1e9, 2), hbm_mb=round(2 * esize * cells / 1e6, 1))
    res["lds_bound_ms"] = round(8 * taps.size * cells / (256 * CUS * GHZ * 1e9) * 1e3, 3)
    res["fp64_bound_ms"] = round(2 * taps.size * cells / (64 * CUS * GHZ * 1e9) * 1e3, 3)
    call = lambda: G.path_enhance(R, N, window="hann", n_filters=N_FILTERS)  # noqa: E731
    res["shipped_ms"] = median_ms(call, iters)
    rounds = {t: [] for t in tiles}
    for t in tiles:   # (warm-up: code objects, the LDS attribute)
        at_tile(t, call)
    torch.cuda.synchronize()
    for _ in range(iters):   # alternating rounds
        for t in tiles:
            rounds[t].append(at_tile(t, lambda: timed_ms(call)))
    res["tiles_ms"] = {f"{t[0]}x{t[1]}": [round(float(np.median(v)), 3), round(float(np.min(v)), 3)] for t, v in rounds.items()}   # [median, min]
    res["best_tile"] = min(res["tiles_ms"], key=lambda k: res["tiles_ms"][k][0])
    res["of_fp64_bound"] = round(res["fp64_bound_ms"] / res["shipped_ms"], 3)
    # the lag view of the same matrix: t x t in, 2t x t out
    traffic = 3 * esize * cells
    res["lag_ms"] = median_ms(lambda: G.recurrence_to_lag(R), iters)
    res["lag_axis0_ms"] = median_ms(lambda: G.recurrence_to_lag(R, axis=0), iters)
    res["lag_gbps"] = round(traffic / res["lag_ms"] / 1e6, 1)
    res["lag_axis0_gbps"] = round(traffic / res["lag_axis0_ms"] / 1e6, 1)
    res["copy_gbps"] = copy_gbps(traffic, iters)
    res["lag_of_copy"] = round(res["lag_gbps"] / res["copy_gbps"], 3)
    res["lag_axis0_of_copy"] = round(res["lag_axis0_gbps"] / res["copy_gbps"], 3)
    return res


def stack(iters, gen):
    d, t, steps = 12, 4_000_000, 10
    x = torch.rand((d, t), dtype=torch.float32, device="cuda", generator=gen)
    traffic = 4 * d * t * (1 + steps)
    res = dict(shape=[d, t], n_steps=steps, traffic_mb=round(traffic / 1e6, 1))
    res["stack_ms"] = median_ms(lambda: F.stack_memory(x, n_steps=steps, delay=3), iters)
    res["stack_gbps"] = round(traffic / res["stack_ms"] / 1e6, 1)
    res["copy_gbps"] = copy_gbps(traffic, iters)
    res["stack_of_copy"] = round(res["stack_gbps"] / res["copy_gbps"], 3)
    return res


def scipy_baseline(side=1292):
    import scipy.ndimage

    R = np.random.default_rng(3).random((side, side))
    t0 = time.perf_counter()
    out = None
    for r in np.logspace(-1, 1, num=N_FILTERS, base=2):
        resp = scipy.ndimage.convolve(R, filters.diagonal_filter("hann", N, slope=r))
        out = resp if out is None else np.maximum(out, resp, out=out)
    np.clip(out, 0, None, out=out)
    return dict(side=side, scipy_ndimage_s=round(time.perf_counter() - t0, 3), threads_available=len(os.sched_getaffinity(0)))


def main():
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 5
    gen = torch.Generator(device="cuda").manual_seed(7)
    if "--once" in sys.argv:
        R = torch.rand((1292, 1292), dtype=torch.float64, device="cuda", generator=gen)
        for _ in range(2):
            G.path_enhance(R, N, window="hann", n_filters=N_FILTERS)
            G.recurrence_to_lag(R)
            torch.cuda.synchronize()
        return
    res = {}
    for side in (1292,) if "--small" in sys.argv else (1292, 12920):
        for dtype in (torch.float64, torch.float32):
            key = f"{side}_{str(dtype).split('.')[-1]}"
            res[key] = enhance(side, dtype, iters, gen, TILES if side == 1292 else TILES[:3])
            print(json.dumps({key: res[key]}), flush=True)
    res["stack_memory"] = stack(iters, gen)
    print(json.dumps({"stack_memory": res["stack_memory"]}), flush=True)
    res["baseline"] = scipy_baseline()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
