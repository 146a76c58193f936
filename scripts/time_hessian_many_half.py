"""Timing of the grouped GPTQ Hessian on half-precision activations, one process, one device (HIP events).

    python scripts/time_hessian_many_half.py [--calls 20 --warmup 5]

Workload: one gemma-3-270m-shaped calibration batch, 72 tapped inputs of [10, 512, 640 / 1024 / 2048] (5120 rows each), as fp16 and
as bf16, every Hessian already holding 10 samples (H is read and written, as from the second batch on).  Per element type,
milliseconds per batch (one pair of events per batch, median and minimum over the calls) for
  (a) the grouped fp32 chain (`oq_hessian_accumulate_many_f32`) on fp32 copies made outside the timed region;
  (b) what a holder of half activations had before the grouped half chain: `ops.hessian_accumulate` per tensor, forked over four
      side streams and joined -- the calibration driver's route, call for call;
  (c) the grouped half chain (`ops.hessian_accumulate_many` on the half tensors: one `oq_hessian_accumulate_many_h16` call).
The results of (b) and (c) are compared with each other and (c) with (a) before anything is timed.  Prints one JSON line.  Exits
non-zero when the median of (c) is not below the median of (b) for both types: that is a condition.  (c) below (a) is a target:
reported, not asserted."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from onnx_quantize_amd.hip import ops  # noqa: E402

WIDTHS = [640, 640, 1024, 2048] * 18
SEEN = 10


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3)}


def side_stream_route(xs, hs, side):
    """ActivationStream.feed's per-tensor route: fork by an event, one `ops.hessian_accumulate` per tensor round-robin over the side
    streams, join."""
    cur = torch.cuda.current_stream()
    fork = cur.record_event()
    for i, (x, h) in enumerate(zip(xs, hs)):
        s = side[i % len(side)]
        s.wait_event(fork)
        with torch.cuda.stream(s):
            ops.hessian_accumulate(x, h, SEEN)
        x.record_stream(s)
    for s in side:
        cur.wait_stream(s)


def one(dtype, calls, warmup):
    g = torch.Generator(device="cuda").manual_seed(2)
    xs = [(torch.randn((10, 512, k), generator=g, device="cuda") * (0.1 + 3.9 * torch.rand(k, generator=g, device="cuda"))).to(dtype) for k in WIDTHS]
    xs32 = [x.float() for x in xs]
    side = [torch.cuda.Stream() for _ in range(4)]
    seen = [SEEN] * len(xs)
    base = [torch.randn((k, k), generator=g, device="cuda") for k in WIDTHS]
    base = [b + b.T for b in base]
    hs = {r: [b.clone() for b in base] for r in "abc"}
    ops.hessian_accumulate_many(xs32, hs["a"], seen)
    side_stream_route(xs, hs["b"], side)
    ops.hessian_accumulate_many(xs, hs["c"], seen)
    torch.cuda.synchronize()
    b_vs_c = max(float((b - c).abs().max() / b.abs().max()) for b, c in zip(hs["b"], hs["c"]))
    a_vs_c = max(float((a - c).abs().max() / a.abs().max()) for a, c in zip(hs["a"], hs["c"]))
    assert b_vs_c <= 1e-5 and a_vs_c <= 1e-5, f"the routes differ: (b) vs (c) {b_vs_c:.3e}, (a) vs (c) {a_vs_c:.3e} of max |H|"
    res = {"a_fp32_grouped_copies_outside": timed(lambda: ops.hessian_accumulate_many(xs32, hs["a"], seen), calls, warmup),
           "b_per_tensor_four_side_streams": timed(lambda: side_stream_route(xs, hs["b"], side), calls, warmup),
           "c_half_grouped": timed(lambda: ops.hessian_accumulate_many(xs, hs["c"], seen), calls, warmup)}
    res["b_vs_c"] = float(f"{b_vs_c:.3e}")
    res["a_vs_c"] = float(f"{a_vs_c:.3e}")
    res["c_over_b"] = round(res["c_half_grouped"]["median_ms"] / res["b_per_tensor_four_side_streams"]["median_ms"], 3)
    res["c_over_a"] = round(res["c_half_grouped"]["median_ms"] / res["a_fp32_grouped_copies_outside"]["median_ms"], 3)
    res["condition_c_below_b"] = res["c_half_grouped"]["median_ms"] < res["b_per_tensor_four_side_streams"]["median_ms"]
    res["target_c_below_a"] = res["c_half_grouped"]["median_ms"] < res["a_fp32_grouped_copies_outside"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    res = {"tensors": len(WIDTHS), "rows": 5120, "calls": a.calls, "warmup": a.warmup}
    for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        res[name] = one(dtype, a.calls, a.warmup)
        ops.release_workspaces()
        torch.cuda.empty_cache()
    res["condition_c_below_b"] = all(res[n]["condition_c_below_b"] for n in ("fp16", "bf16"))
    res["target_c_below_a"] = all(res[n]["target_c_below_a"] for n in ("fp16", "bf16"))
    print(json.dumps(res))
    if not res["condition_c_below_b"]:
        sys.exit("CONDITION FAILED: the grouped half chain is not faster than per-tensor calls on four side streams")


if __name__ == "__main__":
    main()
