"""Timing of `ops.qlinear_function` / `ops.qlinear_function_decode` (one library call per call of a QLinearMatMul / QLinearGemm
function: fp32 X in, fp32 Y out) against what `GraphRunner` executes for such a call under "fused" / "fused+decode", HIP events, one
device.

    python scripts/time_qlinear_function.py [--calls 20 --warmup 5 --repeats 3 --timeout 240]

uint8 A (static activation parameters) x int8 B with per-column parameters, uint8 Y; [K, N] = 4096 x 11008, 11008 x 4096 and
4096 x 4096; B stored [K, N] (what files hold) and [N, K]; M = 1, 4, 16 on the decode route and M = 2048 on the tile route.  Arms:
  (a) the bare integer call (`ops.qlinear_matmul_decode` / `ops.qlinear_matmul`) on an A quantized outside the timed region, uint8 Y:
      the floor, reported only;
  (b) what the runner executes today: its own `_quantize` (five torch launches), that kernel, its own `_op_DequantizeLinear` (three);
  (c) the new call on the fp32 X (the bytes of (b): checked before anything is timed).
Each arm is measured two ways: EAGER -- warm-ups, then one pair of events around `calls` back-to-back calls, what a Python caller
gets -- and REPLAYED: the `calls` calls captured once into one graph (a linear chain, no parallel branches) and the pair of events
around one replay, which shows the device time.  Every case runs in a child process of its own under `--timeout` seconds; the first
case that fails, faults or times out ends the run.  Inside a case the arms alternate in each of the `repeats` repetitions.  Prints
one JSON line per case -- microseconds per call as the mean of the repetitions and their spread (max - min), (c) over (b), and
(c) - (a) beside the time the extra bytes (X as fp32 in, Y as fp32 out) take at 8 TB/s -- and exits non-zero when the gate fails: on
the two large shapes (c) is below (b) by more than the spread of (b), eager and replayed, at every M and layout.  4096 x 4096 is
reported only."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from time_qlinear_decode import captured, eager, replayed  # noqa: E402  (the same laps)

CASES = [(layout, m, k, n) for layout in ("KN", "NK") for m in (1, 4, 16, 2048) for k, n in ((4096, 11008), (11008, 4096), (4096, 4096))]
PEAK_BYTES = 8e12


def run_case(layout, m, k, n, calls, warmup, repeats):
    import torch

    from onnx_quantize_amd.graph_runner import GraphRunner, _Attrs
    from onnx_quantize_amd.hip import ops

    g = torch.Generator(device="cuda").manual_seed(0)
    trans_b, decode = layout == "NK", m <= 16
    a_s, a_zp = torch.tensor(0.02, device="cuda"), torch.tensor(128, dtype=torch.uint8, device="cuda")
    x = (torch.rand((m, k), device="cuda", generator=g) * 255.0 - 128.0) * 0.02          # every level of the uint8 range
    b = torch.randint(-127, 128, (n, k) if trans_b else (k, n), device="cuda", generator=g, dtype=torch.int32).to(torch.int8)
    b_s = torch.rand((n,), device="cuda", generator=g) * 0.004 + 0.008
    b_zp = torch.randint(-3, 4, (n,), device="cuda", generator=g, dtype=torch.int32).to(torch.int8)
    y_s, y_zp = torch.tensor(0.02 * 0.01 * 74 * 74 * k ** 0.5 / 40, device="cuda"), torch.tensor(128, dtype=torch.uint8, device="cuda")

    runner, no_attrs = GraphRunner.evaluator(21), _Attrs({})
    integer = ops.qlinear_matmul_decode if decode else ops.qlinear_matmul
    function = ops.qlinear_function_decode if decode else ops.qlinear_function
    a = runner._quantize(x, a_s, a_zp)

    def three_nodes():
        q = integer(runner._quantize(x, a_s, a_zp), a_s, a_zp, b, b_s, b_zp, y_s, y_zp, trans_b=trans_b)
        return runner._op_DequantizeLinear(None, [q, y_s, y_zp], no_attrs, None)

    arms = {"a_integer_call_only": lambda: integer(a, a_s, a_zp, b, b_s, b_zp, y_s, y_zp, trans_b=trans_b),
            "b_three_nodes": three_nodes,
            "c_one_call": lambda: function(x, a_s, a_zp, b, b_s, b_zp, y_s, y_zp, trans_b=trans_b)}

    three, one = arms["b_three_nodes"](), arms["c_one_call"]()
    if not torch.equal(three.view(torch.int32), one.view(torch.int32)) or len(torch.unique(one)) < 40:
        print(json.dumps({"layout": layout, "M": m, "K": k, "N": n, "error": "the one call does not give the three nodes' bytes"}), flush=True)
        return 4
    graphs = {name: captured(fn, calls, warmup) for name, fn in arms.items()}
    laps = {(name, how): [] for name in arms for how in ("eager", "replayed")}
    for _ in range(repeats):
        for name, fn in arms.items():
            laps[(name, "eager")].append(eager(fn, calls, warmup) * 1e3)
        for name in arms:
            laps[(name, "replayed")].append(replayed(graphs[name], calls, warmup) * 1e3)
    case = {"layout": layout, "M": m, "K": k, "N": n, "route": "decode" if decode else "tile", "unit": "us per call"}
    for (name, how), v in laps.items():
        case.setdefault(name, {})[how] = {"mean_us": round(sum(v) / len(v), 2), "spread_us": round(max(v) - min(v), 2)}
    gated = (k, n) != (4096, 4096)
    met = True
    for how in ("eager", "replayed"):
        aa, bb, cc = (case[name][how] for name in arms)
        case[f"c_over_b_{how}"] = round(cc["mean_us"] / bb["mean_us"], 3)
        case[f"c_minus_a_{how}_us"] = round(cc["mean_us"] - aa["mean_us"], 2)
        met = met and cc["mean_us"] < bb["mean_us"] - bb["spread_us"]
    case["extra_bytes_at_8_TBs_us"] = round((m * k * 4 + m * n * 4) / PEAK_BYTES * 1e6, 2)
    case["gate"] = "c < b - spread(b), eager and replayed" if gated else "reported only"
    case["gate_met"] = met
    print(json.dumps(case), flush=True)
    return 0 if met or not gated else 3


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
