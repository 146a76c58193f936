"""Timing of `ops.qdq_matmul` (the product of a QDQ function run from its stored integers) against the routes it replaces, HIP
events, one device.  The protocol is that of scripts/time_matmul_nbits.py.

    python scripts/time_qdq_matmul.py [--calls 20 --warmup 5 --repeats 3 --timeout 240]

A in fp16 and in fp32; W int8 per column, and int4 values one per byte in groups of 128 along K; M = 2048 and M = 16 on
[K, N] = 11008 x 4096, 4096 x 11008 and 4096 x 4096.  Arms:
  (a) torch.matmul on a weight expanded ONCE outside the timed region (2 to 4 times the stored bytes, kept resident);
  (b) today's route, the function body as `GraphRunner` walks it (onnx_functions.build_function: DequantizeLinear of the whole
      weight -- for groups a cast, two transposes and two reshapes around a blocked one -- then the product), every call.  A
      2-byte A meets the dequantized weight cast to its type, as `GraphRunner._op_MatMulNBits` does;
  (c) ops.qdq_matmul on W as stored.
Every case runs in a child process of its own under `--timeout` seconds; the first case that fails, faults or times out ends the
run.  Inside a case the arms alternate in each of the `repeats` repetitions (warm-ups, then one pair of events around `calls`
back-to-back calls).  Prints one JSON line per case -- milliseconds per call as the mean of the repetitions and their spread
(max - min), the relative Frobenius error of each arm against float64 on 64 output columns, the fraction of the 2.5 PFLOP/s
matrix peak for (c) (an fp32 A counts as two products) and the time W alone takes at 8 TB/s of HBM -- and exits non-zero when
the gate fails: in every case, (c) below (b) by more than the spread of (b).  (c) against (a) is reported, not gated."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(dt, kind, m, k, n) for dt in ("float16", "float32") for kind in ("int8_column", "int4_group128") for m in (2048, 16)
         for k, n in ((11008, 4096), (4096, 11008), (4096, 4096))]
GROUP, PEAK_FLOPS, HBM_BYTES_PER_S = 128, 2.5e15, 8e12


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


def run_case(dt, kind, m, k, n, calls, warmup, repeats):
    import torch

    from onnx_quantize_amd.graph_runner import GraphRunner
    from onnx_quantize_amd.hip import ops
    from onnx_quantize_amd.onnx_functions import build_function

    dtype = getattr(torch, dt)
    g = torch.Generator(device="cuda").manual_seed(0)
    grouped = kind == "int4_group128"
    blocks = k // GROUP if grouped else 1
    lo, hi = (-8, 8) if grouped else (-128, 128)
    w = torch.randint(lo, hi, (k, n), device="cuda", generator=g, dtype=torch.int32).to(torch.int8)
    zp = torch.randint(-3, 4, (n, blocks), device="cuda", generator=g, dtype=torch.int32).to(torch.int8)
    scales = torch.rand((n, blocks), device="cuda", generator=g) * 0.02 + 0.001
    x = torch.randn((m, k), device="cuda", generator=g).to(dtype)
    group_size = GROUP if grouped else 0

    # (b): the body of the function the writer emits, up to its product, walked by the runner's own operators
    fn = build_function("QMatMulWeightsOnlyGrouped", group_size=GROUP, four_bit=True) if grouped else build_function("QMatMulWeightsOnlyQDQ")
    body = [node for node in fn.node if node.op_type != "MatMul"]
    runner = GraphRunner.evaluator(21)
    stored = {"W": w, "w_scale": scales.reshape(-1, 1) if grouped else scales.reshape(n), "w_zero_point": zp.reshape(-1, 1) if grouped else zp.reshape(n),
              "original_transposed_shape": torch.tensor([n, k], dtype=torch.int64)}

    def function_body():
        env = dict(stored)
        runner._run(body, env)
        dequantized = env["dequantized_weights"]
        return torch.matmul(x, dequantized if dequantized.dtype == dtype else dequantized.to(dtype))

    def expanded(rows=slice(None), to=torch.float32):
        d = w.t()[rows].to(to).reshape(-1, blocks, k // blocks) - zp[rows].to(to)[:, :, None]
        return (d * scales[rows].to(to)[:, :, None]).reshape(-1, k)

    resident = expanded().to(dtype).t().contiguous()
    arms = {"a_expanded_outside": lambda: torch.matmul(x, resident), "b_function_body": function_body,
            "c_fused": lambda: ops.qdq_matmul(x, w, scales.reshape(-1), zp.reshape(-1), group_size=group_size)}

    cols = 64
    y64 = x.double() @ expanded(slice(0, cols), torch.float64).t()
    with torch.no_grad():
        errors = {name: ((fn_()[:, :cols].double() - y64).norm() / y64.norm()).item() for name, fn_ in arms.items()}
        laps = {name: [] for name in arms}
        for _ in range(repeats):
            for name, fn_ in arms.items():
                laps[name].append(once(fn_, calls, warmup))
    case = {"a_type": dt, "weights": kind, "M": m, "K": k, "N": n, "unit": "ms per call"}
    for name, v in laps.items():
        case[name] = {"mean_ms": round(sum(v) / len(v), 4), "spread_ms": round(max(v) - min(v), 4), "rel_error_vs_float64": float(f"{errors[name]:.3e}")}
    c, b = case["c_fused"], case["b_function_body"]
    products = 2 if dt == "float32" else 1
    case["c_fraction_of_matrix_peak"] = round(products * 2.0 * m * n * k / (c["mean_ms"] * 1e-3) / PEAK_FLOPS, 4)
    case["w_hbm_ms"] = round(w.numel() / HBM_BYTES_PER_S * 1e3, 4)
    case["c_over_a"] = round(c["mean_ms"] / case["a_expanded_outside"]["mean_ms"], 3)
    case["c_over_b"] = round(c["mean_ms"] / b["mean_ms"], 3)
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
