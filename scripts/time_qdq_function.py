"""Timing of `ops.qdq_function` (one library call per call of a QDQ function with quantized activations: fp32 X in, fp32 Y out, the
product on the int8 matrix cores) against what `GraphRunner` executes for such a call by default and under qdq="fused", HIP events,
one device.

    python scripts/time_qdq_function.py [--calls 20 --warmup 5 --repeats 3 --timeout 240]

uint8 X x int8 W with per-column parameters (MatMul), [K, N] = 4096 x 11008 and 11008 x 4096, M = 2048 and M = 16, the six
combinations of a static / dynamic input with no / a static / a dynamic output Q -> DQ.  Arms:
  (a) the default function body, node by node on torch (the body `build_function` writes; for the two mixed combinations, which no
      function name carries, the input side of one body and the output side of another);
  (b) the "fused" composition: the runner's own input operators, `ops.qdq_matmul` on the fp32 x_dequantized, the runner's own output
      operators;
  (c) `ops.qdq_function`.
Each arm is measured EAGER -- warm-ups, then one pair of events around `calls` back-to-back calls -- and REPLAYED: the `calls` calls
captured once into one graph and the pair of events around one replay.  Every case runs in a child process of its own under
`--timeout` seconds; the first case that faults or times out ends the run.  Inside a case the arms alternate in each of the
`repeats` repetitions.  Prints one JSON line per case -- microseconds per call as the mean of the repetitions and their spread
(max - min) -- and, at the end, what is reported without a gate: (c) beside `ops.qlinear_function` on the same operands for the
static input + output, and the cost of the dynamic launches as differences between cases ((dynamic, o) - (static, o): the min / max
pass and the parameter kernel; (i, dynamic) - (i, none): the finishing launch and the pairs).
GATE (a non-zero exit status): at M = 2048, (c) below (b) by more than (b)'s spread, eager and replayed, in all twelve cells.  M = 16 is
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

COMBOS = [("static", None), ("static", "static"), ("static", "dynamic"), ("dynamic", None), ("dynamic", "static"), ("dynamic", "dynamic")]
CASES = [(m, k, n, combo) for m in (2048, 16) for k, n in ((4096, 11008), (11008, 4096)) for combo in COMBOS]


def body(x_mode, out_mode):
    """The nodes of the MatMul function with this input and output side, and the index of the product."""
    from onnx_quantize_amd.onnx_functions import _MATMUL_QDQ, build_function

    def split(fn):
        nodes = list(fn.node)
        at = next(i for i, n in enumerate(nodes) if n.op_type == "MatMul")
        return nodes, at
    nodes, at = split(build_function(_MATMUL_QDQ[(x_mode, None)]))
    if out_mode:
        tail, tail_at = split(build_function(_MATMUL_QDQ[(None, out_mode)]))
        nodes = nodes + tail[tail_at + 1:]
    return nodes, at


def run_case(m, k, n, combo, calls, warmup, repeats):
    import torch

    from onnx_quantize_amd.graph_runner import GraphRunner
    from onnx_quantize_amd.hip import ops

    x_mode, out_mode = combo
    g = torch.Generator(device="cuda").manual_seed(0)
    x = (torch.rand((m, k), device="cuda", generator=g) * 255.0 - 128.0) * 0.02          # every level of the uint8 range
    w = torch.randint(-127, 128, (k, n), device="cuda", generator=g, dtype=torch.int32).to(torch.int8)
    w_s = torch.rand((n,), device="cuda", generator=g) * 0.004 + 0.008
    w_zp = torch.randint(-3, 4, (n,), device="cuda", generator=g, dtype=torch.int32).to(torch.int8)
    x_s, x_zp = torch.tensor(0.02, device="cuda"), torch.tensor(128, dtype=torch.uint8, device="cuda")
    o_s, o_zp = torch.tensor(0.02 * 0.01 * 74 * 74 * k ** 0.5 / 40, device="cuda"), torch.tensor(128, dtype=torch.uint8, device="cuda")
    given = {"X": x, "W": w, "w_scale": w_s, "w_zero_point": w_zp}
    if x_mode == "static":
        given.update(x_scale=x_s, x_zero_point=x_zp)
    if out_mode == "static":
        given.update(out_scale=o_s, out_zero_point=o_zp)
    nodes, at = body(x_mode, out_mode)
    result = nodes[-1].output[0]
    runner = GraphRunner.evaluator(21)
    runner.matmul = "torch"                                                 # the evaluator sets no product route: torch's, the default

    def default_body():
        env = dict(given)
        runner._run(nodes, env)
        return env[result]

    def fused():
        env = dict(given)
        runner._run(nodes[1:at], env)                                       # the input side; nodes[0] dequantizes W
        env[nodes[at].output[0]] = ops.qdq_matmul(env[nodes[at].input[0]], w, w_s, w_zp)
        runner._run(nodes[at + 1:], env)
        return env[result]

    kw = dict(x_mode=x_mode, x_scale=given.get("x_scale"), x_zero_point=given.get("x_zero_point"), out_mode=out_mode,
              out_scale=given.get("out_scale"), out_zero_point=given.get("out_zero_point"))
    arms = {"a_default_body": default_body, "b_fused": fused, "c_one_call": lambda: ops.qdq_function(x, w, w_s, w_zp, **kw)}
    if combo == ("static", "static"):                                          # the same product on the other operand family's call
        arms["d_qlinear_function"] = lambda: ops.qlinear_function(x, x_s, x_zp, w, w_s, w_zp, o_s, o_zp)

    with torch.no_grad():
        ref, one = arms["b_fused"](), arms["c_one_call"]()
        step = float(o_s) if out_mode == "static" else float(ref.max() - ref.min()) / 255 if out_mode else 1e-3 * float(ref.abs().max())
        apart = float((ref.double() - one.double()).abs().max()) / step
        if not apart <= 2.01 or len(torch.unique(one)) < 40:
            print(json.dumps({"M": m, "K": k, "N": n, "combo": combo, "error": f"the one call is {apart} steps from the fused composition"}), flush=True)
            return 4
        graphs = {name: captured(fn, calls, warmup) for name, fn in arms.items()}
        laps = {(name, how): [] for name in arms for how in ("eager", "replayed")}
        for _ in range(repeats):
            for name, fn in arms.items():
                laps[(name, "eager")].append(eager(fn, calls, warmup) * 1e3)
            for name in arms:
                laps[(name, "replayed")].append(replayed(graphs[name], calls, warmup) * 1e3)
    case = {"M": m, "K": k, "N": n, "x_mode": x_mode, "out_mode": out_mode, "unit": "us per call", "steps_from_fused": round(apart, 3)}
    for (name, how), v in laps.items():
        case.setdefault(name, {})[how] = {"mean_us": round(sum(v) / len(v), 2), "spread_us": round(max(v) - min(v), 2)}
    gated, met = m == 2048, True
    for how in ("eager", "replayed"):
        bb, cc = case["b_fused"][how], case["c_one_call"][how]
        case[f"c_over_b_{how}"] = round(cc["mean_us"] / bb["mean_us"], 3)
        case[f"c_over_a_{how}"] = round(cc["mean_us"] / case["a_default_body"][how]["mean_us"], 3)
        met = met and cc["mean_us"] < bb["mean_us"] - bb["spread_us"]
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
    ap.add_argument("--rows", type=int, default=None, help="only the cases of this M")
    a = ap.parse_args()
    if a.case is not None:
        sys.exit(run_case(*CASES[a.case], a.calls, a.warmup, a.repeats))
    failed, seen = [], {}
    for i, case in enumerate(CASES):
        if a.rows is not None and case[0] != a.rows:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(i), "--calls", str(a.calls), "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
        try:
            r = subprocess.run(cmd, timeout=a.timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            sys.exit(f"case {case} ran into its time limit of {a.timeout} s: nothing more is started")
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode == 3:
            failed.append(case)
        elif r.returncode != 0:
            sys.exit(f"case {case} ended with status {r.returncode}: nothing more is started")
        seen[case] = json.loads(r.stdout.strip().splitlines()[-1])
    # reported without a gate: the dynamic launches as differences between cases (replayed: device time)
    for (m, k, n, (x_mode, out_mode)), c in seen.items():
        t = lambda key: seen[key]["c_one_call"]["replayed"]["mean_us"] if key in seen else None      # noqa: E731
        line = {"M": m, "K": k, "N": n, "x_mode": x_mode, "out_mode": out_mode}
        if x_mode == "dynamic" and t((m, k, n, ("static", out_mode))) is not None:
            line["minmax_and_params_us"] = round(t((m, k, n, (x_mode, out_mode))) - t((m, k, n, ("static", out_mode))), 2)
        if out_mode == "dynamic" and t((m, k, n, (x_mode, None))) is not None:
            line["pairs_and_finish_us"] = round(t((m, k, n, (x_mode, out_mode))) - t((m, k, n, (x_mode, None))), 2)
        if "d_qlinear_function" in c:
            line["c_over_qlinear_function_replayed"] = round(c["c_one_call"]["replayed"]["mean_us"] / c["d_qlinear_function"]["replayed"]["mean_us"], 3)
        if len(line) > 5:
            print(json.dumps(line), flush=True)
    if failed:
        sys.exit(f"GATE FAILED: {failed}")


if __name__ == "__main__":
    main()
