"""Timing of RTN on LISTS of half-precision weights (`ops.rtn_quantize_model` -> oq_rtn_quantize_ptrs_h16), HIP events.

    python scripts/time_rtn_many_half.py [--calls 20 --warmup 5 --limit 240]

Two lists, as fp16 and as bf16, uint4 g128, layouts "nbits" and "kn_packed4":
  1. the gemma-3-270m-shaped list bench.py uses for `model_rtn.small_matrices`: 126 weights, 100 M parameters;
  2. 32 matrices of 4096 x 4096 (a call that splits into several launches: ~1.6e8 parameters each).
Milliseconds per list (one pair of events per call, the median over `calls` calls after `warmup` warm-ups) for
  (a) `ops.rtn_quantize_many` on fp32 copies made outside the timed region;
  (b) the per-matrix `ops.rtn_quantize` loop on the half tensors: what a holder of a half model had before;
  (c) `ops.rtn_quantize_model` on the half tensors.
(b) and (c) are measured three times in alternation in the same process; the figure of each is the median of its three
repetitions and the spread of (b) is max - min of its three.  Before anything is timed three sampled entries of (c) are compared
with the single call.

Every step -- one (list, element type), both layouts -- is a child process of its own under its own time limit; the parent never
opens the GPU and stops at the first step that fails.  Prints one JSON line.  Exits non-zero unless, on list 1, (c) is below
(b) by more than the spread of (b) for every type and layout: that is a condition.  (c) <= (a) on both lists is a target:
reported, not asserted."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUP = 128
LAYOUTS = ("nbits", "kn_packed4")
GEMMA = [(640, 1024), (640, 256), (640, 256), (1024, 640), (640, 2048), (640, 2048), (2048, 640)]      # x 18 layers, bench.py
LISTS = {"gemma_126": [sh for _ in range(18) for sh in GEMMA], "32_of_4096x4096": [(4096, 4096)] * 32}
STEPS = [(name, dt) for name in LISTS for dt in ("fp16", "bf16")]


def timed(torch, fn, calls, warmup):
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
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def step(name, dt, calls, warmup):
    import torch

    from onnx_quantize_amd.hip import ops

    dtype = torch.float16 if dt == "fp16" else torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(3)
    ws = [(torch.randn(sh, generator=gen, device="cuda") * 0.05).to(dtype) for sh in LISTS[name]]
    ws32 = [w.float() for w in ws]
    res = {"matrices": len(ws), "params": sum(w.numel() for w in ws)}
    for layout in LAYOUTS:
        a_fn = lambda: ops.rtn_quantize_many(ws32, "uint4", GROUP, layout=layout)                                   # noqa: E731
        b_fn = lambda: [ops.rtn_quantize(w, "uint4", "group", GROUP, layout=layout) for w in ws]                    # noqa: E731
        c_fn = lambda: ops.rtn_quantize_model(ws, "uint4", GROUP, layout=layout)                                    # noqa: E731
        got = c_fn()
        for i in (0, len(ws) // 2, len(ws) - 1):
            one = ops.rtn_quantize(ws[i], "uint4", "group", GROUP, layout=layout)
            assert all(torch.equal(x, y) for x, y in zip(got[i], one)), f"entry {i} of the list call differs from the single call"
        del got
        a_ms = timed(torch, a_fn, calls, warmup)
        b_ms, c_ms = [], []
        for _ in range(3):
            b_ms.append(timed(torch, b_fn, calls, warmup))
            c_ms.append(timed(torch, c_fn, calls, warmup))
        b, c, spread = statistics.median(b_ms), statistics.median(c_ms), max(b_ms) - min(b_ms)
        res[layout] = {"a_fp32_many_copies_outside_ms": round(a_ms, 3), "b_per_matrix_loop_ms": round(b, 3), "c_rtn_quantize_model_ms": round(c, 3),
                       "b_repetitions_ms": [round(x, 3) for x in b_ms], "c_repetitions_ms": [round(x, 3) for x in c_ms],
                       "b_spread_ms": round(spread, 3), "sampled_entries_equal_single_call": True,
                       "condition_c_below_b_by_more_than_the_spread": bool(b - c > spread), "target_c_not_above_a": bool(c <= a_ms)}
        ops.release_workspaces()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--step", nargs=2, metavar=("LIST", "TYPE"), help="internal: run one step in this process")
    a = ap.parse_args()
    if a.step:
        return step(a.step[0], a.step[1], a.calls, a.warmup)
    res = {"calls": a.calls, "warmup": a.warmup, "qtype": "uint4", "group": GROUP}
    for name, dt in STEPS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--calls", str(a.calls), "--warmup", str(a.warmup), "--step", name, dt],
                           capture_output=True, text=True, timeout=a.limit)
        if r.returncode != 0:      # nothing more is started on the device behind a step that failed
            print(json.dumps(res))
            sys.exit(f"step {name} / {dt} failed with exit code {r.returncode}:\n{r.stdout[-1000:]}\n{r.stderr[-3000:]}")
        res.setdefault(name, {})[dt] = json.loads(r.stdout.strip().splitlines()[-1])
    cells = lambda name: [res[name][dt][lay] for dt in ("fp16", "bf16") for lay in LAYOUTS]      # noqa: E731
    res["condition_list_1_c_below_b_by_more_than_the_spread"] = all(c["condition_c_below_b_by_more_than_the_spread"] for c in cells("gemma_126"))
    res["target_c_not_above_a_on_both_lists"] = all(c["target_c_not_above_a"] for name in LISTS for c in cells(name))
    print(json.dumps(res))
    if not res["condition_list_1_c_below_b_by_more_than_the_spread"]:
        sys.exit("CONDITION FAILED: rtn_quantize_model is not faster than the per-matrix loop on the gemma-shaped list by more than the loop's spread")


if __name__ == "__main__":
    main()
