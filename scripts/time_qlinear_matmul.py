"""Timing of `ops.qlinear_matmul` (QLinearMatMul / QGemm on the int8 matrix cores) against the routes it replaces, HIP events, one device.

    python scripts/time_qlinear_matmul.py [--calls 20 --warmup 5 --repeats 3 --timeout 240]

uint8 A (static activation parameters) x int8 B with per-channel scales; M = 2048 and M = 16 on [K, N] = 4096 x 11008, 11008 x 4096
and 4096 x 4096; B stored [K, N] (QLinearMatMul) and [N, K] (QGemm, transB = 1).  Arms:
  (a) torch.matmul in fp32 on operands dequantized ONCE outside the timed region (the weight at four times its bytes, kept resident);
  (b) the expansion of `GraphRunner._op_QLinearMatMul` / `_op_QGemm` as the runner runs it: both dequantizations, the fp32 product,
      the re-quantization -- what a holder of such a file has without the kernel;
  (c) ops.qlinear_matmul on the operands as stored.
Every case runs in a child process of its own under `--timeout` seconds; the first case that fails, faults or times out ends the
run.  Inside a case the arms alternate in each of the `repeats` repetitions (warm-ups, then one pair of events around `calls`
back-to-back calls).  Prints one JSON line per case -- milliseconds per call as the mean of the repetitions and their spread
(max - min), (c) as a fraction of 5 Pop/s (twice the 2.5 PFLOP/s the README uses for fp16: the int8 matrix instruction has twice the
depth at the same cycles), the share of outputs where (c) and (b) differ and by how many levels at most -- and exits non-zero when
the gate fails: at M = 2048, (c) below (b) by more than the spread of (b).  (c) against (a), and the M = 16 rows, are reported, not
gated."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(layout, m, k, n) for layout in ("KN", "NK") for m in (2048, 16) for k, n in ((4096, 11008), (11008, 4096), (4096, 4096))]
PEAK_OPS = 5e15


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


def run_case(layout, m, k, n, calls, warmup, repeats):
    import torch

    from onnx_quantize_amd.graph_runner import GraphRunner
    from onnx_quantize_amd.hip import ops

    g = torch.Generator(device="cuda").manual_seed(0)
    trans_b = layout == "NK"
    a = torch.randint(0, 256, (m, k), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    b = torch.randint(-127, 128, (n, k) if trans_b else (k, n), device="cuda", generator=g, dtype=torch.int32).to(torch.int8)
    a_s, a_zp = torch.tensor(0.02, device="cuda"), torch.tensor(128, dtype=torch.uint8, device="cuda")
    b_s = torch.rand((n,), device="cuda", generator=g) * 0.004 + 0.008
    b_zp = torch.zeros((n,), dtype=torch.int8, device="cuda")
    y_s, y_zp = torch.tensor(0.02 * 0.01 * 74 * 74 * k ** 0.5 / 40, device="cuda"), torch.tensor(128, dtype=torch.uint8, device="cuda")

    runner = GraphRunner.evaluator(21)
    if trans_b:
        expansion = lambda: GraphRunner._op_QGemm(runner, None, [a, a_s, a_zp, b, b_s, b_zp, None, y_s, y_zp], {"transB": 1}, None)      # noqa: E731
    else:
        expansion = lambda: GraphRunner._op_QLinearMatMul(runner, None, [a, a_s, a_zp, b, b_s, b_zp, y_s, y_zp], {}, None)      # noqa: E731
    a_f = (a.float() - 128.0) * a_s
    b_f = b.float() * (b_s.reshape(-1, 1) if trans_b else b_s.reshape(1, -1))
    arms = {"a_fp32_dequantized_outside": (lambda: torch.matmul(a_f, b_f.t())) if trans_b else (lambda: torch.matmul(a_f, b_f)),
            "b_expansion": expansion,
            "c_fused": lambda: ops.qlinear_matmul(a, a_s, a_zp, b, b_s, b_zp, y_s, y_zp, trans_b=trans_b)}

    apart = (arms["c_fused"]().int() - arms["b_expansion"]().int()).abs()
    laps = {name: [] for name in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            laps[name].append(once(fn, calls, warmup))
    case = {"layout": layout, "M": m, "K": k, "N": n, "unit": "ms per call"}
    for name, v in laps.items():
        case[name] = {"mean_ms": round(sum(v) / len(v), 4), "spread_ms": round(max(v) - min(v), 4)}
    c, bb = case["c_fused"], case["b_expansion"]
    case["c_fraction_of_5_Pops"] = round(2.0 * m * n * k / (c["mean_ms"] * 1e-3) / PEAK_OPS, 4)
    case["c_over_a"] = round(c["mean_ms"] / case["a_fp32_dequantized_outside"]["mean_ms"], 3)
    case["c_over_b"] = round(c["mean_ms"] / bb["mean_ms"], 3)
    case["c_vs_b_outputs_differing"] = round(float((apart != 0).double().mean()), 6)
    case["c_vs_b_max_levels_apart"] = int(apart.max())
    if m == 2048:
        case["gate"] = "c < b - spread(b)"
        case["gate_met"] = c["mean_ms"] < bb["mean_ms"] - bb["spread_ms"]
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
