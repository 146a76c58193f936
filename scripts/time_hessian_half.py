"""Timing of the GPTQ Hessian on half-precision activations against the two fp32 routes, one process, one device (HIP events).

    python scripts/time_hessian_half.py [--rows 65536 --widths 11008 4096 --calls 20 --warmup 5]

Per width and element type (fp16, bf16): (a) x.float() made once outside the timed region, then the current default of
`ops.hessian_accumulate` (the fp16-piece method at these sizes); (b) x.float() inside the timed region plus that default -- the
only route a holder of half activations had before oq_hessian_accumulate_h16; (c) the half kernel on x as it is.  The results
of (a) and (c) are compared before anything is timed, and (c) is compared with float64 on 64 sampled columns.  Prints one JSON
line: milliseconds per call (one pair of events per call, median and minimum over the calls), the fraction of the dense fp16 /
bf16 matrix peak (c) reaches on the T K (K + 256) multiply-adds of its upper-triangle tiles, and (c) / (a).  Exits non-zero
when (c) is not faster than (b) everywhere: that is a condition, not a target."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from onnx_quantize_amd.hip import ops  # noqa: E402

MATRIX_PEAK = 2.5e15       # dense fp16 / bf16 MFMA, FLOP/s (16 x the 157.3 TFLOP/s of the fp32 matrix path)


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


def one(rows, k, dtype, calls, warmup):
    torch.manual_seed(k)
    x = (torch.randn((rows, k), device="cuda") * (0.1 + 3 * torch.rand(k, device="cuda"))).to(dtype).reshape(4, rows // 4, k)
    x32 = x.float()
    h = {r: torch.zeros((k, k), device="cuda") for r in "ac"}
    ops.hessian_accumulate(x32, h["a"], 0)
    ops.hessian_accumulate(x, h["c"], 0)
    top = float(h["a"].abs().max())
    agree = float((h["a"] - h["c"]).abs().max()) / top
    assert agree <= 1e-5, f"(a) and (c) differ by {agree:.3e} of max |H|"
    cols = torch.randperm(k, device="cuda")[:64]
    x64 = x.reshape(-1, k).double()
    ref = (2.0 / 4) * (x64.T @ x64[:, cols])
    err64 = float((h["c"][:, cols].double() - ref).abs().max() / ref.abs().max())
    err64_a = float((h["a"][:, cols].double() - ref).abs().max() / ref.abs().max())
    del x64, ref
    res = {"a_fp32_copy_outside": timed(lambda: ops.hessian_accumulate(x32, h["a"], 0), calls, warmup),
           "b_cast_then_fp32_route": timed(lambda: ops.hessian_accumulate(x.float(), h["a"], 0), calls, warmup),
           "c_half_kernel": timed(lambda: ops.hessian_accumulate(x, h["c"], 0), calls, warmup)}
    kp = (k + 255) // 256 * 256
    flop = 2.0 * rows * kp * (kp + 256) / 2            # the upper-triangle tiles, diagonal tiles whole
    res["c_half_kernel"]["fraction_of_matrix_peak"] = round(flop / (res["c_half_kernel"]["median_ms"] * 1e-3) / MATRIX_PEAK, 3)
    res["c_over_a"] = round(res["c_half_kernel"]["median_ms"] / res["a_fp32_copy_outside"]["median_ms"], 3)
    res["c_vs_float64_on_64_columns"] = float(f"{err64:.3e}")
    res["a_vs_float64_on_64_columns"] = float(f"{err64_a:.3e}")
    res["a_vs_c"] = float(f"{agree:.3e}")
    res["c_faster_than_b"] = res["c_half_kernel"]["median_ms"] < res["b_cast_then_fp32_route"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--widths", type=int, nargs="+", default=[11008, 4096])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    res = {"rows": a.rows}
    for k in a.widths:
        for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
            res[f"{k}_{name}"] = one(a.rows, k, dtype, a.calls, a.warmup)
            ops.release_workspaces()
            torch.cuda.empty_cache()
    res["c_faster_than_b"] = all(v["c_faster_than_b"] for v in res.values() if isinstance(v, dict))
    print(json.dumps(res))
    if not res["c_faster_than_b"]:      # (b) moves seven times the bytes and runs three products: a half kernel that loses to it is broken
        sys.exit("CONDITION FAILED: the half kernel is not faster than x.float() followed by the fp32 route")


if __name__ == "__main__":
    main()
