"""Timing of HQQ on a half-precision matrix against the fp32 routes, one process, one device (HIP events).

    python scripts/time_hqq_half.py [--k 4096 --n 11008 --calls 20 --warmup 5 --repeats 3]

uint4, default HqqConfig values (20 rounds, early stop), [K, N] output; fp16 and bf16, group 128 and group 256.  Arms:
  (a) hqq_quantize on an fp32 copy made outside the timed region;
  (b) w.float() + hqq_quantize inside the timed region -- the only route a holder of a 2-byte matrix had before
      oq_hqq_optimize_h16;
  (c) hqq_quantize on the half tensor;
  (d) group 256 only: (c) with per_round_launches=True (W re-read every round: the route group 256 takes for fp32).
The arms alternate inside each of the `repeats` repetitions (warm-ups, then one pair of events around `calls` back-to-back
calls).  Prints one JSON line: milliseconds per call, the mean of the repetitions and their spread (max - min).  Exits non-zero
when a gate fails: (c) below (b) by more than the spread of (b) at group 128, (c) below (d) by more than the spread of (d) at
group 256.  (c) against (a) is reported, not gated."""
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
            ref, got = ops.hqq_quantize(w32, g), ops.hqq_quantize(w, g)
            assert all(torch.equal(x, y) for x, y in zip(ref, got)), "the half result differs from the fp32 kernels'"
            arms = {"a_fp32_copy_outside": lambda: ops.hqq_quantize(w32, g),
                    "b_cast_inside": lambda: ops.hqq_quantize(w.float(), g),
                    "c_half": lambda: ops.hqq_quantize(w, g)}
            if g == 256:
                arms["d_half_per_round"] = lambda: ops.hqq_quantize(w, g, per_round_launches=True)
            laps = {name: [] for name in arms}
            for _ in range(a.repeats):
                for name, fn in arms.items():
                    laps[name].append(once(fn, a.calls, a.warmup))
            case = {name: {"mean_ms": round(sum(v) / len(v), 4), "spread_ms": round(max(v) - min(v), 4)} for name, v in laps.items()}
            case["rounds"] = int(got[3])
            case["c_over_a"] = round(case["c_half"]["mean_ms"] / case["a_fp32_copy_outside"]["mean_ms"], 3)
            against = "b_cast_inside" if g == 128 else "d_half_per_round"
            case["gate"] = f"c < {against[0]} - spread({against[0]})"
            case["gate_met"] = case["c_half"]["mean_ms"] < case[against]["mean_ms"] - case[against]["spread_ms"]
            key = f"{str(dtype).split('.')[-1]}_g{g}"
            res["cases"][key] = case
            if not case["gate_met"]:
                failed.append(key)
    print(json.dumps(res))
    if failed:
        sys.exit(f"GATE FAILED: {', '.join(failed)}")


if __name__ == "__main__":
    main()
