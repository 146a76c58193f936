"""Timing of RTN on a half-precision matrix against the two fp32 routes, one process, one device (HIP events).

    python scripts/time_rtn_half.py [--k 4096 --n 11008 --launches 20 --warmup 5]

uint4, group 128, MatMulNBits blob.  (a) the fp32 kernel on the fp32 copy; (b) w.float() followed by the fp32 kernel -- the
only route a holder of a 2-byte matrix had before oq_rtn_quantize_h16; (c) the half kernel on fp16 and on bf16.  Prints one
JSON line: microseconds per call (events around the launches, median and minimum of five repeats) and the fraction of the HBM peak the half kernel
reaches on its algorithmic bytes (W once at 2 bytes, the blob, scales and zero points).  Exits non-zero when (c) is not
faster than (b): that is a condition, not a target."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from onnx_quantize_amd.hip import ops  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, launches, warmup, repeats=5):
    """Microseconds per call: one pair of events around `launches` back-to-back calls (the host runs ahead of the device, so
    this is device time per call unless the call is host-bound), `repeats` times; median and minimum of the repeats."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / launches)
    return {"median_us": round(statistics.median(out), 2), "min_us": round(min(out), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--n", type=int, default=11008)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    k, n, g = a.k, a.n, 128
    torch.manual_seed(0)
    w16 = torch.randn((k, n), device="cuda", dtype=torch.float32).to(torch.float16)
    wb16 = w16.float().to(torch.bfloat16)
    w32 = w16.float()
    outs = {dt: ops.rtn_quantize(w, "uint4", "group", g, layout="nbits") for dt, w in (("f32", w32), ("f16", w16), ("bf16", wb16))}
    assert all(torch.equal(x, y) for x, y in zip(outs["f32"], outs["f16"])), "fp16 result differs from the fp32 kernel"
    ref_b = ops.rtn_quantize(wb16.float(), "uint4", "group", g, layout="nbits")
    assert all(torch.equal(x, y) for x, y in zip(ref_b, outs["bf16"])), "bf16 result differs from the fp32 kernel"
    run = lambda w, dt: (lambda: ops.rtn_quantize(w, "uint4", "group", g, layout="nbits", out=outs[dt]))
    res = {"shape": [k, n], "group": g,
           "a_fp32_kernel": timed(run(w32, "f32"), a.launches, a.warmup),
           "b_cast_then_fp32_kernel": timed(lambda: ops.rtn_quantize(w16.float(), "uint4", "group", g, layout="nbits", out=outs["f32"]),
                                            a.launches, a.warmup),
           "c_half_kernel_fp16": timed(run(w16, "f16"), a.launches, a.warmup),
           "c_half_kernel_bf16": timed(run(wb16, "bf16"), a.launches, a.warmup)}
    nbytes = k * n * 2 + k * n // 2 + (k // g) * n * 5
    res["half_algorithmic_bytes"] = nbytes
    for key in ("c_half_kernel_fp16", "c_half_kernel_bf16"):
        res[key]["fraction_of_hbm_peak"] = round(nbytes / (res[key]["median_us"] * 1e-6) / HBM_PEAK, 3)
    res["c_faster_than_b"] = max(res["c_half_kernel_fp16"]["median_us"], res["c_half_kernel_bf16"]["median_us"]) < res["b_cast_then_fp32_kernel"]["median_us"]
    print(json.dumps(res))
    if not res["c_faster_than_b"]:      # (b) moves about four times the bytes: a half kernel that loses to it is broken, not slow
        sys.exit("CONDITION FAILED: the half kernel is not faster than w.float() followed by the fp32 kernel")


if __name__ == "__main__":
    main()
