"""Timing of `ops.qdq_function_decode` -- arm (c), the decode route: the [K, N] bytes streamed once -- against `ops.qdq_function` --
arm (b), the tile route, whose sources this route leaves as they are -- on the same operands, HIP events, one device.  The protocol
is that of scripts/time_qdq_function_packed4_decode.py.

    python scripts/time_qdq_function_decode.py [--repeats 5 --window 0.1]

[K, N] = 4096 x 11008 and 11008 x 4096, uint8 per column with zero points; M = 1, 4 and 16; static input / no output Q -> DQ and
dynamic input / dynamic output.  Each case is timed twice: eagerly (the host's cost of a call included: at M <= 4 it is most of the
figure) and as the replay of a captured graph of `GRAPH_CALLS` calls (the device's time).  The two arms alternate in each of the
`repeats` repetitions; a repetition is warm-ups, then one pair of events around as many back-to-back calls (replays) as fill `window`
seconds.  Both arms must give the same bytes, or the run stops.  Prints one JSON line per case: microseconds per call as the mean of
the repetitions and their spread (max - min) for each arm and way, `gate`: (c) is below (b) by more than (b)'s own spread, and the
replayed (c) as a fraction of 8 TB/s on the algorithmic bytes (W + X + Y)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES, ROWS, HBM_BYTES_PER_S, GRAPH_CALLS = [(4096, 11008), (11008, 4096)], (1, 4, 16), 8e12, 20
CELLS = [("static", None), ("dynamic", "dynamic")]


def once(fn, calls, warmup=3):
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
    return a.elapsed_time(b) * 1e3 / calls


def replayed(fn):
    """`GRAPH_CALLS` calls of `fn` as one captured graph: (its replay, the output of the last call)."""
    import torch
    fn()                                           # the workspace sizes are asked for outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(GRAPH_CALLS):
            out = fn()
    return graph.replay, out


def run_case(k, n, x_mode, out_mode, m, repeats, window):
    import torch

    from onnx_quantize_amd.hip import ops

    g = torch.Generator(device="cuda").manual_seed(0)
    w = torch.randint(0, 256, (k, n), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    zp = torch.randint(120, 136, (n,), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    scales = torch.rand((n,), device="cuda", generator=g) * 0.02 + 0.001
    x = torch.randn((m, k), device="cuda", generator=g)
    kw = dict(x_mode=x_mode, out_mode=out_mode)
    if x_mode == "static":
        kw.update(x_scale=torch.tensor(0.03, device="cuda"), x_zero_point=torch.tensor(128, dtype=torch.uint8, device="cuda"))
    arms = {"b_tile": lambda: ops.qdq_function(x, w, scales, zp, **kw), "c_decode": lambda: ops.qdq_function_decode(x, w, scales, zp, **kw)}
    want = arms["b_tile"]().view(torch.uint8)
    if not torch.equal(want, arms["c_decode"]().view(torch.uint8)):
        sys.exit(f"{k}x{n} {x_mode} {out_mode} M={m}: the two routes give different bytes")
    case = {"K": k, "N": n, "x_mode": x_mode, "out_mode": out_mode, "M": m, "unit": "us per call"}
    for way in ("eager", "replay"):
        runs, per = dict(arms), 1
        if way == "replay":
            per = GRAPH_CALLS
            for name, fn in arms.items():
                runs[name], out = replayed(fn)
                runs[name]()
                torch.cuda.synchronize()
                if not torch.equal(want, out.view(torch.uint8)):
                    sys.exit(f"{k}x{n} {x_mode} {out_mode} M={m}: the replay of {name} gives other bytes than its eager call")
        calls = {name: max(5, int(window * 1e6 / once(fn, 5))) for name, fn in runs.items()}
        laps = {name: [] for name in runs}
        for _ in range(repeats):
            for name, fn in runs.items():
                laps[name].append(once(fn, calls[name]) / per)
        for name, v in laps.items():
            case[f"{way}_{name}"] = {"mean_us": round(sum(v) / len(v), 2), "spread_us": round(max(v) - min(v), 2)}
        b, c = case[f"{way}_b_tile"], case[f"{way}_c_decode"]
        case[f"{way}_gate"] = b["mean_us"] - c["mean_us"] > b["spread_us"]
    least = (w.numel() + x.numel() * 4 + m * n * 4) / HBM_BYTES_PER_S * 1e6
    case["algorithmic_bytes_us_at_8TBs"] = round(least, 2)
    case["replay_c_fraction_of_8TBs"] = round(least / case["replay_c_decode"]["mean_us"], 3)
    print(json.dumps(case), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1, help="seconds of back-to-back calls per repetition and arm")
    a = ap.parse_args()
    for k, n in SHAPES:
        for x_mode, out_mode in CELLS:
            for m in ROWS:
                run_case(k, n, x_mode, out_mode, m, a.repeats, a.window)


if __name__ == "__main__":
    main()
