"""Timing of `ops.matmul_nbits_float_zp` (a MatMulNBits node with float zero points run from its blob past 16 rows) against the
route it replaces, HIP events, one device.

    python scripts/time_matmul_nbits_fzp.py [--calls 20 --warmup 5 --repeats 3 --timeout 240]

uint4, group size 128, float32 zero points as HQQ leaves them (mid-range, fractional); A in fp16, bf16 and fp32; M = 2048 and M = 64
on [N, K] = 4096 x 11008, 11008 x 4096 and 4096 x 4096.  Arms:
  (b) the arithmetic of `GraphRunner._op_MatMulNBits` with the expansion inside -- where such a node went before;
  (c) ops.matmul_nbits_float_zp on the blob as stored;
  (i) ops.matmul_nbits on the same blob with the zero points rounded (rint) and packed: NOT the same product -- the yardstick of
      what the kernel costs without the correction;
  (a) torch.matmul on a weight expanded ONCE outside the timed region (4 to 8 times the blob's memory, kept resident).
Every case runs in a child process of its own under `--timeout` seconds; the first case that fails, faults or times out ends the
run.  Inside a case the arms alternate in each of the `repeats` repetitions (warm-ups, then one pair of events around `calls`
back-to-back calls).  Prints one JSON line per case -- milliseconds per call as the mean of the repetitions and their spread
(max - min), the relative Frobenius error of (a), (b) and (c) against float64 on 64 output columns -- and exits non-zero when the
gate fails: in every case, (c) below (b) by more than the spread of (b).  (c) / (i), the price of the correction (one more MFMA
per four and a second fma in the fold: at most 1.25 of the matrix instructions), and (c) / (a) are reported, not gated."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(dt, m, n, k) for dt in ("float16", "bfloat16", "float32") for m in (2048, 64) for n, k in ((4096, 11008), (11008, 4096), (4096, 4096))]
GROUP, BITS = 128, 4


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
    zp = 7.5 + (torch.rand((n, blocks), device="cuda", generator=g) - 0.5) * 2
    zi = torch.round(zp).clamp_(0, 15).to(torch.uint8)
    zi_packed = (zi[:, 0::2] | (zi[:, 1::2] << 4)).contiguous()
    scales = (torch.rand((n, blocks), device="cuda", generator=g) * 0.02 + 0.001).to(dtype)
    x = torch.randn((m, k), device="cuda", generator=g).to(dtype)

    runner = GraphRunner.evaluator(21)
    attrs = {"K": k, "N": n, "bits": BITS, "block_size": GROUP}
    expand_inside = lambda: GraphRunner._op_MatMulNBits(runner, None, [x, blob, scales, zp], attrs, None)      # noqa: E731
    w = ((q.float() - zp[:, :, None]) * scales.float()[:, :, None]).reshape(n, k).to(dtype).t().contiguous()
    arms = {"b_expansion_inside": expand_inside,
            "c_float_zp": lambda: ops.matmul_nbits_float_zp(x, blob, scales, zp, K=k, N=n, bits=BITS, block_size=GROUP),
            "i_integer_kernel": lambda: ops.matmul_nbits(x, blob, scales, zi_packed, K=k, N=n, bits=BITS, block_size=GROUP),
            "a_expanded_outside": lambda: torch.matmul(x, w)}

    cols = 64
    w64 = ((q[:cols].double() - zp[:cols].double()[:, :, None]) * scales[:cols].double()[:, :, None]).reshape(cols, k)
    y64 = x.double() @ w64.t()
    errors = {name: ((fn()[:, :cols].double() - y64).norm() / y64.norm()).item() for name, fn in arms.items() if name != "i_integer_kernel"}
    del w64

    laps = {name: [] for name in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            laps[name].append(once(fn, calls, warmup))
    case = {"a_type": dt, "M": m, "N": n, "K": k, "unit": "ms per call"}
    for name, v in laps.items():
        case[name] = {"mean_ms": round(sum(v) / len(v), 4), "spread_ms": round(max(v) - min(v), 4)}
        if name in errors:
            case[name]["rel_error_vs_float64"] = float(f"{errors[name]:.3e}")
    c, b = case["c_float_zp"], case["b_expansion_inside"]
    case["c_over_b"] = round(c["mean_ms"] / b["mean_ms"], 3)
    case["c_over_i"] = round(c["mean_ms"] / case["i_integer_kernel"]["mean_ms"], 3)
    case["c_over_a"] = round(c["mean_ms"] / case["a_expanded_outside"]["mean_ms"], 3)
    case["gate"] = "c < b - spread(b)"
    case["gate_met"] = c["mean_ms"] < b["mean_ms"] - b["spread_ms"]
    print(json.dumps(case), flush=True)
    return 0 if case["gate_met"] else 3


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
