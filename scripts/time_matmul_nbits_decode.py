"""Timing of `ops.matmul_nbits_decode` (the decode route of MatMulNBits, M <= 16) against the routes a caller had before it, HIP
events, one device, by the method of scripts/time_matmul_nbits.py.

    python scripts/time_matmul_nbits_decode.py [--calls 20 --warmup 5 --repeats 3 --timeout 240]

uint4, group size 128, packed zero points, on [N, K] = 4096 x 11008, 11008 x 4096 and 4096 x 4096, M in {1, 4, 16}, A in fp16, bf16
and fp32; and one HQQ-style case (float zero points) on 4096 x 11008 at M = 1, fp16.  Arms:
  (b) ops.matmul_nbits, the tile kernel: the only fused route of the parent commit (not for float zero points, which it refuses);
  (c) ops.matmul_nbits_decode;
  (e) the expansion route of `GraphRunner._op_MatMulNBits`.
Every case runs in a child process of its own under `--timeout` seconds; the first case that fails, faults or times out ends the
run.  Inside a case the arms alternate in each of the `repeats` repetitions (warm-ups, then one pair of events around `calls`
back-to-back calls).  Prints one JSON line per case -- milliseconds per call as the mean of the repetitions and their spread
(max - min), and for (c) the fraction of the 8 TB/s HBM peak on the algorithmic bytes (blob + scales + zero points + A + Y) -- and
exits non-zero when the gate fails: (c) below (b) by more than (b)'s spread in every case; in the HQQ case (c) below (e) by more
than (e)'s spread."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(dt, m, n, k, False) for dt in ("float16", "bfloat16", "float32") for n, k in ((4096, 11008), (11008, 4096), (4096, 4096)) for m in (1, 4, 16)]
CASES.append(("float16", 1, 4096, 11008, True))      # HQQ: float zero points
GROUP, BITS, HBM_BYTES_PER_S = 128, 4, 8e12


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


def run_case(dt, m, n, k, float_zp, calls, warmup, repeats):
    import torch

    from onnx_quantize_amd.graph_runner import GraphRunner
    from onnx_quantize_amd.hip import ops

    dtype = getattr(torch, dt)
    g = torch.Generator(device="cuda").manual_seed(0)
    blocks = k // GROUP
    q = torch.randint(0, 16, (n, blocks, GROUP), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    blob = (q[..., 0::2] | (q[..., 1::2] << 4)).contiguous()
    if float_zp:
        zero_points = torch.rand((n, blocks), device="cuda", generator=g) * 15.0
    else:
        zp = torch.randint(0, 16, (n, blocks), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
        zero_points = (zp[:, 0::2] | (zp[:, 1::2] << 4)).contiguous()
    scales = (torch.rand((n, blocks), device="cuda", generator=g) * 0.02 + 0.001).to(dtype)
    x = torch.randn((m, k), device="cuda", generator=g).to(dtype)
    del q

    runner = GraphRunner.evaluator(21)
    attrs = {"K": k, "N": n, "bits": BITS, "block_size": GROUP}
    kw = dict(K=k, N=n, bits=BITS, block_size=GROUP)
    arms = {"c_decode": lambda: ops.matmul_nbits_decode(x, blob, scales, zero_points, **kw),
            "e_expansion": lambda: GraphRunner._op_MatMulNBits(runner, None, [x, blob, scales, zero_points], attrs, None)}
    if not float_zp:
        arms["b_tile"] = lambda: ops.matmul_nbits(x, blob, scales, zero_points, **kw)

    laps = {name: [] for name in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            laps[name].append(once(fn, calls, warmup))
    case = {"a_type": dt, "M": m, "N": n, "K": k, "float_zero_points": float_zp, "unit": "ms per call"}
    for name, v in sorted(laps.items()):
        case[name] = {"mean_ms": round(sum(v) / len(v), 5), "spread_ms": round(max(v) - min(v), 5)}
    c = case["c_decode"]
    elem = x.element_size()
    algorithmic = blob.numel() + scales.numel() * scales.element_size() + zero_points.numel() * zero_points.element_size() + (m * k + m * n) * elem
    case["algorithmic_bytes"] = algorithmic
    case["hbm_floor_ms"] = round(algorithmic / HBM_BYTES_PER_S * 1e3, 5)
    case["c_fraction_of_hbm_peak"] = round(algorithmic / (c["mean_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
    against = "e_expansion" if float_zp else "b_tile"
    case["gate"] = f"c < {against[0]} - spread({against[0]})"
    case["gate_met"] = c["mean_ms"] < case[against]["mean_ms"] - case[against]["spread_ms"]
    print(json.dumps(case), flush=True)
    assert c["mean_ms"] > 0
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
    assert not failed, f"GATE FAILED: {failed}"


if __name__ == "__main__":
    main()
