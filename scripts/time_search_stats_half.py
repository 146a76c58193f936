"""Timing of the AWQ / SmoothQuant search statistics on half-precision activations, one process, one device (HIP events).

    python scripts/time_search_stats_half.py [--calls 20 --warmup 5]

Workload: one gemma-3-270m-shaped calibration batch, 72 tapped inputs of 5120 rows x 640 / 1024 / 2048 columns, as fp16 and as
bf16, folded into 72 `ops.SearchStatistics` that already hold a batch.  Per element type, milliseconds per batch (one pair of events
per batch, the median over the calls) for
  (a) `SearchStatistics.add_many` on fp32 copies made outside the timed region;
  (b) what a holder of half activations had before: `add_many(stats, [x.float() for x in xs])`, the casts timed;
  (c) `add_many` on the half tensors (one `oq_abs_stats_cols_many_h16` call, the grouped half Hessian chain, no fp32 copy),
each for the whole update and for the |x| part alone (the column sums and maxima, without the Gram matrices).  (b) and (c) are
measured three times in alternation.  `abs_sum` and `absmax` of (b) and (c) are compared bit for bit before anything is timed.
Prints one JSON line.  Exits non-zero unless, for both types, the whole update of (c) is below that of (b) by more than the spread
(max - min) of (b)'s three repetitions: that is a condition.  The |x| part of (c) at or below that of (a) is a target: reported, not
asserted."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from onnx_quantize_amd.hip import _lib as L  # noqa: E402
from onnx_quantize_amd.hip import ops  # noqa: E402

WIDTHS = [640, 640, 1024, 2048] * 18
ROWS = 5120


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
    return round(statistics.median(out), 3)


def abs_part_fp32(stats, xs32):
    """The |x| part of `SearchStatistics.add_many` for fp32 tensors, call for call."""
    lib = L.load()
    for st, x2 in zip(stats, xs32):
        t, k = x2.shape
        ws = ops._workspace(lib.oq_abs_sum_cols_workspace_bytes(k), x2.device)
        L.check(lib.oq_abs_sum_cols_f32(x2.data_ptr(), t, k, x2.stride(0), st.abs_sum.data_ptr(), 1, ws.data_ptr(), ws.numel(),
                                        torch.cuda.current_stream().cuda_stream))
        st.absmax = torch.maximum(st.absmax, ops.absmax(x2))


def abs_part_half(stats, xs):
    ops.abs_stats_accumulate_many(xs, [st.abs_sum for st in stats], [st.absmax for st in stats])


def one(dtype, calls, warmup):
    g = torch.Generator(device="cuda").manual_seed(2)
    xs = [(torch.randn((ROWS, k), generator=g, device="cuda") * (0.1 + 3.9 * torch.rand(k, generator=g, device="cuda"))).to(dtype) for k in WIDTHS]
    xs32 = [x.float() for x in xs]
    stats = {r: [ops.SearchStatistics(k, "cuda") for k in WIDTHS] for r in "abc"}
    ops.SearchStatistics.add_many(stats["a"], xs32)
    ops.SearchStatistics.add_many(stats["b"], [x.float() for x in xs])
    ops.SearchStatistics.add_many(stats["c"], xs)
    torch.cuda.synchronize()
    for b, c in zip(stats["b"], stats["c"]):
        assert torch.equal(b.abs_sum, c.abs_sum) and torch.equal(b.absmax, c.absmax) and b.rows == c.rows, "the routes differ in the |x| statistics"
    gram = max(float((b.gram - c.gram).abs().max() / b.gram.abs().max()) for b, c in zip(stats["b"], stats["c"]))
    assert gram <= 1e-5, f"the Gram matrices of (b) and (c) differ by {gram:.3e} of max |H|"
    routes = {
        "a": (lambda: ops.SearchStatistics.add_many(stats["a"], xs32), lambda: abs_part_fp32(stats["a"], xs32)),
        "b": (lambda: ops.SearchStatistics.add_many(stats["b"], [x.float() for x in xs]), lambda: abs_part_fp32(stats["b"], [x.float() for x in xs])),
        "c": (lambda: ops.SearchStatistics.add_many(stats["c"], xs), lambda: abs_part_half(stats["c"], xs)),
    }
    res = {"a_fp32_copies_outside": {"whole_ms": timed(routes["a"][0], calls, warmup), "abs_ms": timed(routes["a"][1], calls, warmup)}}
    reps = {"b": {"whole_ms": [], "abs_ms": []}, "c": {"whole_ms": [], "abs_ms": []}}
    for _ in range(3):                                     # (b) and (c) in alternation
        for r in "bc":
            reps[r]["whole_ms"].append(timed(routes[r][0], calls, warmup))
            reps[r]["abs_ms"].append(timed(routes[r][1], calls, warmup))
    for r, name in (("b", "b_casts_timed"), ("c", "c_half")):
        res[name] = {part: {"median_ms": statistics.median(v), "repetitions_ms": v} for part, v in reps[r].items()}
    spread = round(max(reps["b"]["whole_ms"]) - min(reps["b"]["whole_ms"]), 3)
    res["b_spread_ms"] = spread
    res["b_vs_c_gram"] = float(f"{gram:.3e}")
    res["condition_c_below_b_by_more_than_the_spread"] = res["b_casts_timed"]["whole_ms"]["median_ms"] - res["c_half"]["whole_ms"]["median_ms"] > spread
    res["target_abs_part_c_at_or_below_a"] = res["c_half"]["abs_ms"]["median_ms"] <= res["a_fp32_copies_outside"]["abs_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    res = {"tensors": len(WIDTHS), "rows": ROWS, "calls": a.calls, "warmup": a.warmup}
    for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        res[name] = one(dtype, a.calls, a.warmup)
        ops.release_workspaces()
        torch.cuda.empty_cache()
    cond = "condition_c_below_b_by_more_than_the_spread"
    res[cond] = all(res[n][cond] for n in ("fp16", "bf16"))
    res["target_abs_part_c_at_or_below_a"] = all(res[n]["target_abs_part_c_at_or_below_a"] for n in ("fp16", "bf16"))
    print(json.dumps(res))
    if not res[cond]:
        sys.exit("CONDITION FAILED: add_many on half tensors is not faster than add_many on timed fp32 casts by more than the spread")


if __name__ == "__main__":
    main()
