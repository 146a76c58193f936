"""Wall time of one eager `GraphRunner` pass over a file with many initializers and many routed function calls, at 5 rows, where
the pass is bound by the runner's Python dispatch and not by its kernels.  One device.

    python scripts/time_runner_dispatch.py [--blocks 67 --passes 40 --warmup 10 --tree DIR]

The file is built here: `blocks` copies, chained, of the two-layer model of tests/test_qdq_function_packed4_runner_gpu.py -- a
static-input MatMul on an INT4 W [64, 48], a dynamic-input Gemm on a UINT4 W [48, 64], a static-input MatMul on an INT4 W with an
odd N -- so 67 blocks are 201 calls of QDQ functions over 1072 initializers.  Measured with every mode "torch" and with
qdq="fused+integer+packed4": `warmup` passes, then `passes` passes, each between two host clock reads with a device synchronise
before either; the median is reported.  The same file is then run with capture=True: the pass has to be recorded and to replay
bit-identically (a non-zero exit status otherwise).  `--tree` times the package of another checkout (a parent commit beside this
one) with the same script; compare medians only against the spread of two runs of the same tree.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

K, N1, N3 = 64, 48, 33
FUNCTIONS = ["QMatMulWeightStaticInputQDQ", "QGemmWeightDynamicInputQDQ"]


def chained(blocks):
    import numpy as np

    from onnx_quantize_amd import onnx_proto as P
    from onnx_quantize_amd.onnx_functions import build_function
    rng = np.random.default_rng(5)
    inits, nodes, outputs = [], [], []

    def weight(name, k, n, code, scales):
        lo, box = (-8, np.int8) if code == P.DataType.INT4 else (0, np.uint8)
        inits.extend([P.numpy_to_tensor(name, rng.integers(lo, lo + 16, (k, n)).astype(box), code), P.numpy_to_tensor(name + "_s", rng.choice(np.float32(scales), n)),
                      P.numpy_to_tensor(name + "_z", rng.integers(lo, lo + 16, n).astype(box), code)])
        return [name, name + "_s", name + "_z"]

    x = "x"
    for b in range(blocks):
        w1, w2, w3 = weight(f"W1_{b}", K, N1, P.DataType.INT4, (1 / 64, 1 / 32)), weight(f"W2_{b}", N1, K, P.DataType.UINT4, (1 / 64, 1 / 32)), \
            weight(f"W3_{b}", N1, N3, P.DataType.INT4, (0.5, 1.0))
        inits.extend([P.numpy_to_tensor(f"B_{b}", rng.integers(-8, 9, K).astype(np.int8)), P.numpy_to_tensor(f"B_s_{b}", np.float32(1.0)),
                      P.numpy_to_tensor(f"B_z_{b}", np.int8(0)), P.numpy_to_tensor(f"x_s_{b}", np.float32(1.0)), P.numpy_to_tensor(f"x_z_{b}", np.uint8(128)),
                      P.numpy_to_tensor(f"h_s_{b}", np.float32(0.5)), P.numpy_to_tensor(f"h_z_{b}", np.uint8(128))])
        nodes += [P.make_node(FUNCTIONS[0], [x, *w1, f"x_s_{b}", f"x_z_{b}"], [f"h_{b}"], domain="quant"),
                  P.make_node(FUNCTIONS[1], [f"h_{b}", w2[0], f"B_{b}", *w2[1:], f"B_s_{b}", f"B_z_{b}"], [f"out_{b}"], domain="quant"),
                  P.make_node(FUNCTIONS[0], [f"h_{b}", *w3, f"h_s_{b}", f"h_z_{b}"], [f"odd_{b}"], domain="quant")]
        outputs.append(f"odd_{b}")
        x = f"out_{b}"
    g = P.Message("GraphProto", name="chained", node=nodes, initializer=inits, input=[P.make_value_info("x", P.DataType.FLOAT, ["M", K])],
                  output=[P.make_value_info(o, P.DataType.FLOAT, None) for o in [x] + outputs])
    model = P.Message("ModelProto", ir_version=10, graph=g, functions=[build_function(f) for f in FUNCTIONS],
                      opset_import=[P.Message("OperatorSetIdProto", domain="", version=21), P.Message("OperatorSetIdProto", domain="quant", version=1)])
    return P.parse_model(P.serialize(model)), len(nodes), len(inits)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=67)
    ap.add_argument("--passes", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package is timed")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch

    from onnx_quantize_amd.graph_runner import GraphRunner
    assert torch.cuda.is_available(), "this timing needs a GPU"
    model, calls, initializers = chained(a.blocks)
    feed = {"x": torch.randint(-2, 3, (5, K), generator=torch.Generator().manual_seed(5)).float().cuda()}
    line = {"tree": os.path.abspath(a.tree), "calls": calls, "initializers": initializers, "rows": 5, "passes": a.passes, "unit": "ms per eager pass, median"}
    for qdq in ("torch", "fused+integer+packed4"):
        runner = GraphRunner(model, device="cuda", qdq=qdq)
        laps = []
        for i in range(a.warmup + a.passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = runner(feed)
            torch.cuda.synchronize()
            laps.append((time.perf_counter() - t0) * 1e3)
        laps = laps[a.warmup:]
        line[qdq] = {"median_ms": round(statistics.median(laps), 3), "min_ms": round(min(laps), 3), "max_ms": round(max(laps), 3),
                     "qdq_function_calls": dict(runner.qdq_function_calls), "qdq_calls": dict(runner.qdq_calls)}
        recorded = GraphRunner(model, device="cuda", qdq=qdq, capture=True)
        replays = [recorded(feed) for _ in range(5)]                          # eager, recorded, then three replays
        same = all(torch.equal(r[name], out[name]) for r in replays for name in out)
        line[qdq]["recorded"] = all(v is not None for v in recorded._graphs.values()) and len(recorded._graphs) == 1
        line[qdq]["replays_bit_identical"] = same
    print(json.dumps(line), flush=True)
    if not all(line[q]["recorded"] and line[q]["replays_bit_identical"] for q in ("torch", "fused+integer+packed4")):
        sys.exit("a pass was not recorded, or a replay differs from the eager pass")


if __name__ == "__main__":
    main()
