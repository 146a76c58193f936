"""Timing of `ops.matmul_nbits` (a MatMulNBits node run from its blob) against the routes it replaces, HIP events, one device.

    python scripts/time_matmul_nbits.py [--calls 20 --warmup 5 --repeats 3 --timeout 240]

uint4, group size 128, packed zero points; A in fp16 and in fp32; M = 2048 on [N, K] = 4096 x 11008, 11008 x 4096 and 4096 x 4096,
and M = 1 and M = 16 on the first.  Arms:
  (a) torch.matmul on a weight expanded ONCE outside the timed region (4 to 8 times the blob's memory, kept resident);
  (b) the arithmetic of `GraphRunner._op_MatMulNBits` with the expansion inside -- what a holder of a quantized file had;
  (c) ops.matmul_nbits on the blob as stored.
Every case runs in a child process of its own under `--timeout` seconds; the first case that fails, faults or times out ends the
run.  Inside a case the arms alternate in each of the `repeats` repetitions (warm-ups, then one pair of events around `calls`
back-to-back calls).  Prints one JSON line per case -- milliseconds per call as the mean of the repetitions and their spread
(max - min), the relative Frobenius error of each arm against float64 on 64 output columns, the fraction of the 2.5 PFLOP/s
matrix peak for (c) (an fp32 A counts as two products) and the time the blob alone takes at 8 TB/s of HBM -- and exits non-zero
when the gate fails: at M = 2048, (c) below (b) by more than the spread of (b).  (c) against (a), and the M = 1 / 16 rows, are
reported, not gated."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(dt, m, n, k) for dt in ("float16", "float32") for m, n, k in
         ((2048, 4096, 11008), (2048, 11008, 4096), (2048, 4096, 4096), (1, 4096, 11008), (16, 4096, 11008))]
GROUP, BITS, PEAK_FLOPS, HBM_BYTES_PER_S = 128, 4, 2.5e15, 8e12


def once(fn, calls, warmup):
    """Milliseconds per call: one pair of events around `calls` back-to-back calls after `warmup` untimed ones."""
    import torch
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


def run_case(dt, m, n, k, calls, warmup, repeats):
    import torch

    from onnx_quantize_amd.graph_runner import GraphRunner
    from onnx_quantize_amd.hip import ops

    dtype = getattr(torch, dt)
    g = torch.Generator(device="cuda").manual_seed(0)
    blocks = k // GROUP
    q = torch.randint(0, 16, (n, blocks, GROUP), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    blob = (q[..., 0::2] | (q[..., 1::2] << 4)).contiguous()
    zp = torch.randint(0, 16, (n, blocks), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    zp_packed = (zp[:, 0::2] | (zp[:, 1::2] << 4)).contiguous()
    scales = (torch.rand((n, blocks), device="cuda", generator=g) * 0.02 + 0.001).to(dtype)
    x = torch.randn((m, k), device="cuda", generator=g).to(dtype)

    runner = GraphRunner.evaluator(21)
    attrs = {"K": k, "N": n, "bits": BITS, "block_size": GROUP}
    expand_inside = lambda: GraphRunner._op_MatMulNBits(runner, None, [x, blob, scales, zp_packed], attrs, None)      # noqa: E731
    w = ((q.float() - zp.float()[:, :, None]) * scales.float()[:, :, None]).reshape(n, k).to(dtype).t().contiguous()
    arms = {"a_expanded_outside": lambda: torch.matmul(x, w), "b_expansion_inside": expand_inside,
            "c_fused": lambda: ops.matmul_nbits(x, blob, scales, zp_packed, K=k, N=n, bits=BITS, block_size=GROUP)}

    cols = 64
    w64 = ((q[:cols].double() - zp[:cols].double()[:, :, None]) * scales[:cols].double()[:, :, None]).reshape(cols, k)
    y64 = x.double() @ w64.t()
    errors = {name: ((fn()[:, :cols].double() - y64).norm() / y64.norm()).item() for name, fn in arms.items()}
    del w64

    laps = {name: [] for name in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            laps[name].append(once(fn, calls, warmup))
    case = {"a_type": dt, "M": m, "N": n, "K": k, "unit": "ms per call"}
    for name, v in laps.items():
        case[name] = {"mean_ms": round(sum(v) / len(v), 4), "spread_ms": round(max(v) - min(v), 4), "rel_error_vs_float64": float(f"{errors[name]:.3e}")}
    c, b = case["c_fused"], case["b_expansion_inside"]
    products = 2 if dt == "float32" else 1
    case["c_fraction_of_matrix_peak"] = round(products * 2.0 * m * n * k / (c["mean_ms"] * 1e-3) / PEAK_FLOPS, 4)
    case["blob_hbm_ms"] = round(blob.numel() / HBM_BYTES_PER_S * 1e3, 4)
    case["c_over_a"] = round(c["mean_ms"] / case["a_expanded_outside"]["mean_ms"], 3)
    case["c_over_b"] = round(c["mean_ms"] / b["mean_ms"], 3)
    if m == 2048:
        case["gate"] = "c < b - spread(b)"
        case["gate_met"] = c["mean_ms"] < b["mean_ms"] - b["spread_ms"]
    print(json.dumps(case), flush=True)
    return 0 if case.get("gate_met", True) else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a case may take")
    ap.add_argument("--case", type=int, default=None, help="run this entry of CASES in this process")
    a = ap.parse_args()
    if a.case is not None:
        sys.exit(run_case(*CASES[a.case], a.calls, a.warmup, a.repeats))
    failed = []
    for i, case in enumerate(CASES):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(i), "--calls", str(a.calls), "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
        try:
            rc = subprocess.run(cmd, timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"case {case} ran into its time limit of {a.timeout} s: nothing more is started")
        if rc == 3:
            failed.append(case)
        elif rc != 0:
            sys.exit(f"case {case} ended with status {rc}: nothing more is started")
    if failed:
        sys.exit(f"GATE FAILED: {failed}")


if __name__ == "__main__":
    main()
