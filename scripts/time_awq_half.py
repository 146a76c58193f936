"""Timing of the AWQ searches on a half-precision weight against the fp32 routes, one process, one device (HIP events).

    python scripts/time_awq_half.py [--k 4096 --n 4096 --t 4096 --calls 20 --warmup 5 --repeats 3]

uint4, group 128 (the fused quantize-residual kernel); fp16 and bf16; the scale search (20 candidates) and the clip search (10) on
both routes: array ``x`` with `t` rows (T < 3 K: the pieces route, where W is two thirds of that kernel's traffic) and running
statistics (the Gram route, where the fp32 difference D dominates).  Arms:
  (a) the search on an fp32 copy of the weight made outside the timed region;
  (b) w.float() + the search inside the timed region -- what every search did with a 2-byte weight before the `_h16` entry points;
  (c) the search on the half tensor.
The arms alternate inside each of the `repeats` repetitions (warm-ups, then one pair of events around `calls` back-to-back
calls; every call ends in the host's read of the winner, so the window covers whole searches).  Prints one JSON line: milliseconds
per call, the mean of the repetitions and their spread (max - min).  Exits non-zero when a gate fails: (c) below (b) by more than
the spread of (b), per case.  (c) against (a) is the target and is reported, not gated."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from onnx_quantize_amd.hip import ops  # noqa: E402


def once(fn, calls, warmup):
    """Milliseconds per call: one pair of events around `calls` back-to-back calls after `warmup` untimed ones."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def same(x, y):
    first = torch.equal(x[0], y[0]) if isinstance(x[0], torch.Tensor) else x[0] == y[0]
    return first and np.array_equal(x[1], y[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--t", type=int, default=4096)
    ap.add_argument("--g", type=int, default=128)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch.manual_seed(0)
    base = torch.randn((a.k, a.n), device="cuda", dtype=torch.float32) * 0.05
    x = torch.randn((a.t, a.k), device="cuda", dtype=torch.float32) * (0.1 + 3.9 * torch.rand(a.k, device="cuda"))
    stats = ops.SearchStatistics(a.k, "cuda")
    stats.add(x)
    cfg = ("uint4", "group", a.g)
    searches = {
        "scale_array": lambda w: ops.awq_scale_search(x, w, *cfg),
        "clip_array": lambda w: ops.awq_clip_search(x, w, *cfg),
        "scale_stats": lambda w: ops.awq_scale_search_stats(stats, w, *cfg),
        "clip_stats": lambda w: ops.awq_clip_search_stats(stats, w, *cfg),
    }
    res = {"shape": [a.t, a.k, a.n], "group": a.g, "calls": a.calls, "warmup": a.warmup, "repeats": a.repeats, "unit": "ms per call", "cases": {}}
    failed = []
    for dtype in (torch.float16, torch.bfloat16):
        w = base.to(dtype)
        w32 = w.float()
        for sname, search in searches.items():
            assert same(search(w32), search(w)), "the half result differs from the fp32 kernels'"
            arms = {"a_fp32_copy_outside": lambda: search(w32), "b_cast_inside": lambda: search(w.float()), "c_half": lambda: search(w)}
            laps = {name: [] for name in arms}
            for _ in range(a.repeats):
                for name, fn in arms.items():
                    laps[name].append(once(fn, a.calls, a.warmup))
            case = {name: {"mean_ms": round(sum(v) / len(v), 4), "spread_ms": round(max(v) - min(v), 4)} for name, v in laps.items()}
            case["c_over_a"] = round(case["c_half"]["mean_ms"] / case["a_fp32_copy_outside"]["mean_ms"], 3)
            case["c_over_b"] = round(case["c_half"]["mean_ms"] / case["b_cast_inside"]["mean_ms"], 3)
            case["gate"] = "c < b - spread(b)"
            case["gate_met"] = case["c_half"]["mean_ms"] < case["b_cast_inside"]["mean_ms"] - case["b_cast_inside"]["spread_ms"]
            key = f"{str(dtype).split('.')[-1]}_{sname}"
            res["cases"][key] = case
            if not case["gate_met"]:
                failed.append(key)
    print(json.dumps(res))
    if failed:
        sys.exit(f"GATE FAILED: {', '.join(failed)}")


if __name__ == "__main__":
    main()
