"""Timing of `ops.qlinear_matmul_decode` (the decode route of QLinearMatMul / QGemm, M = 1 ... 16) against the tile route it stands
next to, HIP events, one device.

    python scripts/time_qlinear_decode.py [--calls 20 --warmup 5 --repeats 3 --timeout 240]

uint8 A (static activation parameters) x int8 B with per-column parameters, uint8 output; M = 1, 4, 16 on [K, N] = 4096 x 11008,
11008 x 4096 and 4096 x 4096; B stored [K, N] (QLinearMatMul) and [N, K] (QGemm, transB = 1).  Arms:
  (a) torch.matmul in fp32 on operands dequantized ONCE outside the timed region (the weight at four times its bytes, kept resident);
  (b) ops.qlinear_matmul, the tile route: what a caller has at these M without the decode route;
  (c) ops.qlinear_matmul_decode on the same operands (the bytes of (b): checked before anything is timed).
Each arm is measured two ways: EAGER -- warm-ups, then one pair of events around `calls` back-to-back calls, what a Python caller
gets, at these sizes mostly the host's time per call -- and REPLAYED: the `calls` calls captured once into one graph (a linear chain,
no parallel branches) and the pair of events around one replay, which shows the device time.  Every case runs in a child process of
its own under `--timeout` seconds; the first case that fails, faults or times out ends the run.  Inside a case the arms alternate in
each of the `repeats` repetitions.  Prints one JSON line per case -- milliseconds per call as the mean of the repetitions and their
spread (max - min), (c) over (a) and (b), and under replay the fraction of 8 TB/s that (c) reaches on the algorithmic bytes (B once,
A, Y) -- and exits non-zero when the gate fails: on the two large shapes (c) is below (b) by more than the spread of (b), eager and
replayed, at every M and layout.  4096 x 4096 is reported only."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(layout, m, k, n) for layout in ("KN", "NK") for m in (1, 4, 16) for k, n in ((4096, 11008), (11008, 4096), (4096, 4096))]
PEAK_BYTES = 8e12


def eager(fn, calls, warmup):
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


def captured(fn, calls, warmup):
    """One graph of `calls` calls in a row, recorded after `warmup` calls on the recording stream."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(calls):
            fn()
    torch.cuda.synchronize()
    return graph


def replayed(graph, calls, warmup):
    """Milliseconds per call: one pair of events around one replay of the graph, after a replay that is not timed."""
    import torch
    graph.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def run_case(layout, m, k, n, calls, warmup, repeats):
    import torch

    from onnx_quantize_amd.hip import ops

    g = torch.Generator(device="cuda").manual_seed(0)
    trans_b = layout == "NK"
    a = torch.randint(0, 256, (m, k), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    b = torch.randint(-127, 128, (n, k) if trans_b else (k, n), device="cuda", generator=g, dtype=torch.int32).to(torch.int8)
    a_s, a_zp = torch.tensor(0.02, device="cuda"), torch.tensor(128, dtype=torch.uint8, device="cuda")
    b_s = torch.rand((n,), device="cuda", generator=g) * 0.004 + 0.008
    b_zp = torch.randint(-3, 4, (n,), device="cuda", generator=g, dtype=torch.int32).to(torch.int8)
    y_s, y_zp = torch.tensor(0.02 * 0.01 * 74 * 74 * k ** 0.5 / 40, device="cuda"), torch.tensor(128, dtype=torch.uint8, device="cuda")

    a_f = (a.float() - 128.0) * a_s
    b_f = (b.float() - (b_zp.float().reshape(-1, 1) if trans_b else b_zp.float().reshape(1, -1))) * (b_s.reshape(-1, 1) if trans_b else b_s.reshape(1, -1))
    arms = {"a_fp32_dequantized_outside": (lambda: torch.matmul(a_f, b_f.t())) if trans_b else (lambda: torch.matmul(a_f, b_f)),
            "b_tile": lambda: ops.qlinear_matmul(a, a_s, a_zp, b, b_s, b_zp, y_s, y_zp, trans_b=trans_b),
            "c_decode": lambda: ops.qlinear_matmul_decode(a, a_s, a_zp, b, b_s, b_zp, y_s, y_zp, trans_b=trans_b)}

    tile, decode = arms["b_tile"](), arms["c_decode"]()
    if not torch.equal(tile, decode) or len(torch.unique(decode)) < 40:
        print(json.dumps({"layout": layout, "M": m, "K": k, "N": n, "error": "the decode route does not give the tile route's bytes"}), flush=True)
        return 4
    graphs = {name: captured(fn, calls, warmup) for name, fn in arms.items()}
    laps = {(name, how): [] for name in arms for how in ("eager", "replayed")}
    for _ in range(repeats):
        for name, fn in arms.items():
            laps[(name, "eager")].append(eager(fn, calls, warmup))
        for name in arms:
            laps[(name, "replayed")].append(replayed(graphs[name], calls, warmup))
    case = {"layout": layout, "M": m, "K": k, "N": n, "unit": "ms per call"}
    for (name, how), v in laps.items():
        case.setdefault(name, {})[how] = {"mean_ms": round(sum(v) / len(v), 5), "spread_ms": round(max(v) - min(v), 5)}
    gated = (k, n) != (4096, 4096)
    met = True
    for how in ("eager", "replayed"):
        aa, bb, cc = (case[name][how] for name in arms)
        case[f"c_over_a_{how}"] = round(cc["mean_ms"] / aa["mean_ms"], 3)
        case[f"c_over_b_{how}"] = round(cc["mean_ms"] / bb["mean_ms"], 3)
        met = met and cc["mean_ms"] < bb["mean_ms"] - bb["spread_ms"]
    case["c_fraction_of_8_TBs_replayed"] = round((k * n + m * k + m * n) / (case["c_decode"]["replayed"]["mean_ms"] * 1e-3) / PEAK_BYTES, 4)
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
