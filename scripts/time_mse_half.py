"""Timing of the MSE range search on a half-precision matrix against the fp32 routes, one process, one device (HIP events).

    python scripts/time_mse_half.py [--k 4096 --n 11008 --calls 20 --warmup 5 --repeats 3]

uint4, group strategy, [K, N] output; fp16 and bf16, group 128 (the register tile) and group 256 (the packed tile; the fp32
search re-reads W per candidate there).  Arms:
  (a) rtn_quantize(mse=True) on an fp32 copy made outside the timed region;
  (b) w.float() + rtn_quantize(mse=True) inside the timed region -- the only route a holder of a 2-byte matrix had before
      oq_rtn_mse_h16;
  (c) rtn_quantize(mse=True) on the half tensor.
The arms alternate inside each of the `repeats` repetitions (warm-ups, then one pair of events around `calls` back-to-back
calls).  Prints one JSON line: milliseconds per call, the mean of the repetitions and their spread (max - min).  Exits non-zero
when a gate fails: (c) below (b) by more than the spread of (b), at both group sizes.  (c) against (a) is the target and is
reported, not gated."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

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
    return torch.equal(x[0], y[0]) and torch.equal(x[1].view(torch.int32), y[1].view(torch.int32)) and torch.equal(x[2], y[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--n", type=int, default=11008)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch.manual_seed(0)
    base = torch.randn((a.k, a.n), device="cuda", dtype=torch.float32)
    res = {"shape": [a.k, a.n], "calls": a.calls, "warmup": a.warmup, "repeats": a.repeats, "unit": "ms per call", "cases": {}}
    failed = []
    for dtype in (torch.float16, torch.bfloat16):
        w = base.to(dtype)
        w32 = w.float()
        for g in (128, 256):
            search = lambda t: ops.rtn_quantize(t, "uint4", "group", g, mse=True)      # noqa: E731
            assert same(search(w32), search(w)), "the half result differs from the fp32 kernels'"
            arms = {"a_fp32_copy_outside": lambda: search(w32), "b_cast_inside": lambda: search(w.float()), "c_half": lambda: search(w)}
            laps = {name: [] for name in arms}
            for _ in range(a.repeats):
                for name, fn in arms.items():
                    laps[name].append(once(fn, a.calls, a.warmup))
            case = {name: {"mean_ms": round(sum(v) / len(v), 4), "spread_ms": round(max(v) - min(v), 4)} for name, v in laps.items()}
            case["c_over_a"] = round(case["c_half"]["mean_ms"] / case["a_fp32_copy_outside"]["mean_ms"], 3)
            case["gate"] = "c < b - spread(b)"
            case["gate_met"] = case["c_half"]["mean_ms"] < case["b_cast_inside"]["mean_ms"] - case["b_cast_inside"]["spread_ms"]
            key = f"{str(dtype).split('.')[-1]}_g{g}"
            res["cases"][key] = case
            if not case["gate_met"]:
                failed.append(key)
    print(json.dumps(res))
    if failed:
        sys.exit(f"GATE FAILED: {', '.join(failed)}")


if __name__ == "__main__":
    main()
