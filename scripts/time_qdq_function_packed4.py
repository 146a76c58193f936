"""Timing of `ops.qdq_function_packed4` (W as packed nibbles, [K, N / 2] bytes) against `ops.qdq_function` on the same integers
unpacked to one value per byte ([K, N] bytes), HIP events, one device.  The protocol is that of scripts/time_qdq_matmul_packed4.py.

    python scripts/time_qdq_function_packed4.py [--repeats 5 --window 0.2]

[K, N] = 4096 x 11008, INT4 per column with zero points; M = 1, 16 and 2048; a static and a dynamic input Q -> DQ, each with no output
Q -> DQ and with a dynamic one.  The two arms alternate in each of the `repeats` repetitions; a repetition is warm-ups, then one pair
of events around as many back-to-back calls as fill `window` seconds.  Both arms must give the same bytes, or the run stops.  Prints
one JSON line per case: microseconds per call as the mean of the repetitions and their spread (max - min) for each arm, packed over
bytes, the time each arm's W alone takes at 8 TB/s of HBM, and `slower_beyond_spread`: the packed arm is slower by more than the
larger of the two spreads.  Nothing is gated."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, N, HBM_BYTES_PER_S = 4096, 11008, 8e12
CASES = [(x_mode, out_mode, m) for x_mode in ("static", "dynamic") for out_mode in (None, "dynamic") for m in (1, 16, 2048)]


def once(fn, calls, warmup=5):
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


def run_case(x_mode, out_mode, m, repeats, window):
    import torch

    from onnx_quantize_amd.hip import ops

    g = torch.Generator(device="cuda").manual_seed(0)
    w = torch.randint(-8, 8, (K, N), device="cuda", generator=g, dtype=torch.int32).to(torch.int8)
    zp = torch.randint(-3, 4, (N,), device="cuda", generator=g, dtype=torch.int32).to(torch.int8)
    scales = torch.rand((N,), device="cuda", generator=g) * 0.02 + 0.001
    x = torch.randn((m, K), device="cuda", generator=g)
    packed = ((w[:, 0::2] & 0x0F) | (w[:, 1::2] << 4)).view(torch.uint8).contiguous()
    kw = dict(x_mode=x_mode, out_mode=out_mode)
    if x_mode == "static":
        kw.update(x_scale=torch.tensor(0.03, device="cuda"), x_zero_point=torch.tensor(128, dtype=torch.uint8, device="cuda"))
    arms = {"bytes": lambda: ops.qdq_function(x, w, scales, zp, **kw), "packed4": lambda: ops.qdq_function_packed4(x, packed, scales, zp, n=N, signed=True, **kw)}
    if not torch.equal(arms["bytes"]().view(torch.uint8), arms["packed4"]().view(torch.uint8)):
        sys.exit(f"{x_mode} {out_mode} M={m}: the two routes give different bytes")
    calls = {name: max(20, int(window * 1e6 / once(fn, 20))) for name, fn in arms.items()}
    laps = {name: [] for name in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            laps[name].append(once(fn, calls[name]))
    case = {"x_mode": x_mode, "out_mode": out_mode, "M": m, "K": K, "N": N, "unit": "us per call", "calls_per_repetition": calls}
    for name, v in laps.items():
        case[name] = {"mean_us": round(sum(v) / len(v), 2), "spread_us": round(max(v) - min(v), 2)}
    b, p = case["bytes"], case["packed4"]
    case["w_hbm_us"] = {"bytes": round(w.numel() / HBM_BYTES_PER_S * 1e6, 2), "packed4": round(packed.numel() / HBM_BYTES_PER_S * 1e6, 2)}
    case["packed4_over_bytes"] = round(p["mean_us"] / b["mean_us"], 3)
    case["slower_beyond_spread"] = p["mean_us"] - b["mean_us"] > max(p["spread_us"], b["spread_us"])
    print(json.dumps(case), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per repetition and arm")
    a = ap.parse_args()
    for x_mode, out_mode, m in CASES:
        run_case(x_mode, out_mode, m, a.repeats, a.window)


if __name__ == "__main__":
    main()
