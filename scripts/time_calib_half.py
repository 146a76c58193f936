"""Timing of calibration ranges (min / max) on half-precision activations against the two fp32 routes, one process, one device
(HIP events).

    python scripts/time_calib_half.py [--elements 650000000 --calls 20 --warmup 5]

Two workloads per element type (fp16, bf16): (i) ONE large tensor through `ops.minmax_collect`; (ii) one gemma-3-270m-shaped
calibration batch -- 72 tapped tensors of [10, 512, 640 | 1024 | 2048] -- through `ops.minmax_collect_many`.  Three conditions
each: (a) the fp32 kernel on an fp32 copy made once outside the timed region; (b) x.float() inside the timed region plus the
fp32 kernel -- the only route a holder of half activations had before oq_minmax_collect_h16; (c) the half kernel on x as it
is.  The states of (a) and (c) are compared bit for bit before anything is timed.  Prints one JSON line: microseconds per call
(one pair of events per call, median and minimum over the calls), bytes per second on 2 bytes per element for (c) and on 4 for
(a), both as fractions of the 8 TB/s HBM peak.  Exits non-zero when (c) is not faster than (b) everywhere: that is a condition;
(c) reaching (a)'s fraction of the peak is a target and only reported."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from onnx_quantize_amd.hip import ops  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s


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
        out.append(a.elapsed_time(b) * 1e3)
    return {"median_us": round(statistics.median(out), 1), "min_us": round(min(out), 1)}


def report(res, elements):
    for key, width in (("a_fp32_copy_outside", 4), ("c_half_kernel", 2)):
        rate = elements * width / (res[key]["median_us"] * 1e-6)
        res[key]["TB_per_s"] = round(rate / 1e12, 3)
        res[key]["fraction_of_hbm_peak"] = round(rate / HBM_PEAK, 3)
    res["c_over_b"] = round(res["c_half_kernel"]["median_us"] / res["b_cast_then_fp32_kernel"]["median_us"], 3)
    res["c_faster_than_b"] = res["c_half_kernel"]["median_us"] < res["b_cast_then_fp32_kernel"]["median_us"]
    res["c_reaches_the_fraction_of_a"] = res["c_half_kernel"]["fraction_of_hbm_peak"] >= res["a_fp32_copy_outside"]["fraction_of_hbm_peak"]
    return res


def same_bits(a, c):
    assert torch.equal(a[:3].view(torch.int32), c[:3].view(torch.int32)), (a.tolist(), c.tolist())


def one_tensor(elements, dtype, calls, warmup):
    x = torch.empty(elements, dtype=dtype, device="cuda").normal_()
    x32 = x.float()
    sa, sc = ops.minmax_state("cuda"), ops.minmax_state("cuda")
    ops.minmax_collect(x32, sa)
    ops.minmax_collect(x, sc)
    same_bits(sa, sc)
    res = {"elements": elements,
           "a_fp32_copy_outside": timed(lambda: ops.minmax_collect(x32, sa), calls, warmup),
           "b_cast_then_fp32_kernel": timed(lambda: ops.minmax_collect(x.float(), sa), calls, warmup),
           "c_half_kernel": timed(lambda: ops.minmax_collect(x, sc), calls, warmup)}
    return report(res, elements)


def gemma_batch(dtype, calls, warmup):
    # bench_calib.py's batch: 18 layers x {attention input and MLP input [10, 512, 640], o_proj input [10, 512, 1024], down_proj
    # input [10, 512, 2048]}: 72 tensors of 6.5 to 21 MB in half
    widths = [640, 640, 1024, 2048] * 18
    xs = [torch.empty((10, 512, w), dtype=dtype, device="cuda").normal_() for w in widths]
    xs32 = [x.float() for x in xs]
    sa, sc = [ops.minmax_state("cuda") for _ in xs], [ops.minmax_state("cuda") for _ in xs]
    ops.minmax_collect_many(xs32, sa)
    ops.minmax_collect_many(xs, sc)
    for a, c in zip(sa, sc):
        same_bits(a, c)
    elements = sum(x.numel() for x in xs)
    res = {"tensors": len(xs), "elements": elements,
           "a_fp32_copy_outside": timed(lambda: ops.minmax_collect_many(xs32, sa), calls, warmup),
           "b_cast_then_fp32_kernel": timed(lambda: ops.minmax_collect_many([x.float() for x in xs], sa), calls, warmup),
           # what MinMaxCalibrator.collect_many did with a half batch before: a cast and a launch pair per tensor
           "b_per_tensor_cast_and_collect": timed(lambda: [ops.minmax_collect(x.float(), s) for x, s in zip(xs, sa)], calls, warmup),
           "c_half_kernel": timed(lambda: ops.minmax_collect_many(xs, sc), calls, warmup)}
    return report(res, elements)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=650_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    res = {}
    for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        res[f"one_tensor_{name}"] = one_tensor(a.elements, dtype, a.calls, a.warmup)
        ops.release_workspaces()
        torch.cuda.empty_cache()
        res[f"gemma3_270m_batch_{name}"] = gemma_batch(dtype, a.calls, a.warmup)
        ops.release_workspaces()
        torch.cuda.empty_cache()
    res["c_faster_than_b"] = all(v["c_faster_than_b"] for v in res.values() if isinstance(v, dict))
    res["c_reaches_the_fraction_of_a"] = all(v["c_reaches_the_fraction_of_a"] for v in res.values() if isinstance(v, dict))
    print(json.dumps(res))
    if not res["c_faster_than_b"]:      # (b) moves five times the bytes: a half kernel that loses to it is broken
        sys.exit("CONDITION FAILED: the half kernel is not faster than x.float() followed by the fp32 kernel")


if __name__ == "__main__":
    main()
