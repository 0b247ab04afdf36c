"""Performance probe (GPU box): device-tensor sequence.viterbi at pyin's shape, and viterbi_binary.

    python scripts/viterbi_probe.py            # CUDA-event medians of 10 calls after a warm-up, one JSON line
    python scripts/viterbi_probe.py --once     # one call of each after a warm-up (for rocprofv3 --kernel-trace --stats)
    python scripts/viterbi_probe.py --batch 64 --iters 3

Timed end to end (the host's float64 tables and predecessor lists, the prepare kernel, the flag read, the decode): 256 sequences of 1292 steps
over the 1200 states of ``np.kron(transition_loop(2, 0.99), transition_local(600, 121, "triangle"))``, thresholded at 1e-4 (pyin's call) and
as a full search, and ``viterbi_binary`` on 256 x 128 labels x 1292 steps.  Beside the times: the bytes the decode must move (``log_prob``
read once, ``ptr`` written once, one pointer per step walked back) and the candidates per step."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from librosa_amd import sequence as S  # noqa: E402

STATES, STEPS, LABELS = 1200, 1292, 128


def median_ms(fn, iters, warmup=2):
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
    return float(np.median(times)), float(np.min(times))


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    batch, iters = arg("--batch", 256), arg("--iters", 10)
    transition = np.kron(S.transition_loop(2, 0.99), S.transition_local(STATES // 2, 121, window="triangle"))
    gen = torch.Generator(device="cuda").manual_seed(5)
    prob = torch.rand((batch, STATES, STEPS), dtype=torch.float64, device="cuda", generator=gen)
    prob /= prob.sum(dim=-2, keepdim=True)
    pb = torch.rand((batch, LABELS, STEPS), dtype=torch.float64, device="cuda", generator=gen)
    tb = np.array([[0.9, 0.1], [0.3, 0.7]])
    calls = {
        "thresholded": lambda: S.viterbi(prob, transition, transition_min_prob=1e-4),
        "full": lambda: S.viterbi(prob, transition),
        "binary": lambda: S.viterbi_binary(pb, tb),
    }
    if "--only" in sys.argv:
        keep = sys.argv[sys.argv.index("--only") + 1].split(",")
        calls = {k: v for k, v in calls.items() if k in keep}
    if "--once" in sys.argv:
        for _ in range(2):
            for fn in calls.values():
                fn()
                torch.cuda.synchronize()
        return
    pred = int((np.log(transition + np.finfo(np.float64).tiny) >= np.log(1e-4 + np.finfo(np.float64).tiny)).sum(axis=0).max())
    res = {"batch": batch, "states": STATES, "steps": STEPS, "labels": LABELS, "longest_predecessor_list": pred,
           "log_prob_read_mb": round(8e-6 * batch * STATES * STEPS, 1), "ptr_written_mb": round(2e-6 * batch * STATES * STEPS, 1), "ptr_walked_kb": round(2e-3 * batch * STEPS, 1),
           "binary_log_prob_read_mb": round(16e-6 * batch * LABELS * STEPS, 1), "binary_ptr_written_mb": round(4e-6 * batch * LABELS * STEPS, 1)}
    for name, fn in calls.items():
        med, mn = median_ms(fn, iters, warmup=1 if name == "full" else 2)
        res[f"{name}_ms"], res[f"{name}_min_ms"] = round(med, 3), round(mn, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
