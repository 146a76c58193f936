"""`GraphRunner(qdq="fused+packed4")`: the 4-bit weights of a default-format file held as the file's packed nibbles and run on
`ops.qdq_matmul_packed4`.  The file is written here with the functions `onnx_functions` builds: a MatMul (INT4 per column) feeding a
Gemm (UINT4 per column) and a MatMul whose N is odd.  Integers under power-of-two scales keep every fp32 sum of every route exact
(layer 1: |x| <= 2, |q - zp| <= 15, K = 64, scales 1/64, 1/32 -> 12 bits; layer 2: + 4 + 6 + 1 -> 23): the routes must be EQUAL."""
import numpy as np
import pytest
import torch

from onnx_quantize_amd import onnx_proto as P
from onnx_quantize_amd.graph_runner import GraphRunner
from onnx_quantize_amd.onnx_functions import build_function

pytestmark = pytest.mark.gpu
K, N1, N2, N3 = 64, 48, 34, 33


def two_layers():
    rng = np.random.default_rng(3)
    inits = []

    def weight(name, k, n, code, scales):
        lo = -8 if code == P.DataType.INT4 else 0
        box = np.int8 if code == P.DataType.INT4 else np.uint8
        inits.extend([P.numpy_to_tensor(name, rng.integers(lo, lo + 16, (k, n)).astype(box), code),
                      P.numpy_to_tensor(name + "_s", rng.choice(np.float32(scales), n)),
                      P.numpy_to_tensor(name + "_z", rng.integers(lo, lo + 16, n).astype(box), code)])
        return [name, name + "_s", name + "_z"]

    w1, w2, w3 = weight("W1", K, N1, P.DataType.INT4, (1 / 64, 1 / 32)), weight("W2", N1, N2, P.DataType.UINT4, (0.5, 1.0)), \
        weight("W3", N1, N3, P.DataType.INT4, (0.5, 1.0))
    inits.extend([P.numpy_to_tensor("B", rng.integers(-8, 9, N2).astype(np.int8)), P.numpy_to_tensor("B_s", np.float32(1.0)),
                  P.numpy_to_tensor("B_z", np.int8(0))])
    nodes = [P.make_node("QMatMulWeightsOnlyQDQ", ["x", *w1], ["h"], domain="quant"),
             P.make_node("QGemmWeightsOnlyQDQ", ["h", w2[0], "B", *w2[1:], "B_s", "B_z"], ["out"], domain="quant"),
             P.make_node("QMatMulWeightsOnlyQDQ", ["h", *w3], ["odd"], domain="quant")]
    g = P.Message("GraphProto", name="two_layers", node=nodes, initializer=inits, input=[P.make_value_info("x", P.DataType.FLOAT, ["M", K])],
                  output=[P.make_value_info("out", P.DataType.FLOAT, ["M", N2]), P.make_value_info("odd", P.DataType.FLOAT, ["M", N3])])
    model = P.Message("ModelProto", ir_version=10, graph=g, functions=[build_function("QMatMulWeightsOnlyQDQ"), build_function("QGemmWeightsOnlyQDQ")],
                      opset_import=[P.Message("OperatorSetIdProto", domain="", version=21), P.Message("OperatorSetIdProto", domain="quant", version=1)])
    return P.parse_model(P.serialize(model))                  # through the wire, like a file


@pytest.mark.parametrize("rows", [5, 40])
def test_the_packed_runner_holds_the_nibbles_and_gives_the_default_routes_values(rows):
    model = two_layers()
    feed = {"x": torch.randint(-2, 3, (rows, K), generator=torch.Generator().manual_seed(rows)).float()}
    packed, default = GraphRunner(model, device="cuda", qdq="fused+packed4"), GraphRunner(model, device="cuda")
    assert packed.qdq == "fused+packed4" and packed.qdq_calls == {"fused": 0, "torch": 0, "packed4": 0}
    a, b = packed(feed), default(feed)
    assert packed.qdq_calls == {"packed4": 2, "fused": 1, "torch": 0} and default.qdq_calls == {"fused": 0, "torch": 3}
    for name in ("out", "odd"):
        assert a[name].dtype == torch.float32 and torch.equal(a[name], b[name]) and float(b[name].abs().max()) > 1.0, name
    for name, k, n in (("W1", K, N1), ("W2", N1, N2)):
        w = packed.constants[name]
        assert w.dtype == torch.uint8 and w.is_cuda and w.numel() == k * n // 2 and w.shape == (k, n // 2)
        assert torch.equal(GraphRunner._unpacked4(*packed._packed4[id(w)]), default.constants[name])      # what a left-out call would read
    assert packed.constants["W3"].shape == (N1, N3) and torch.equal(packed.constants["W3"], default.constants["W3"])
    only = GraphRunner(model, outputs=["out"], device="cuda", qdq="fused+packed4")
    assert torch.equal(only(feed)["out"], b["out"]) and only.qdq_calls == {"packed4": 2, "fused": 0, "torch": 0}
    with pytest.raises(ValueError, match="fused\\+packed4"):
        GraphRunner(model, device="cuda", qdq="packed4")
    model.graph.node = list(model.graph.node) + [P.make_node("Cast", ["W1"], ["w1_as_float"], to=P.DataType.FLOAT)]      # another reader of W1
    model.graph.output = list(model.graph.output) + [P.make_value_info("w1_as_float", P.DataType.FLOAT, [K, N1])]
    held = GraphRunner(model, device="cuda", qdq="fused+packed4").constants
    assert held["W1"].shape == (K, N1) and held["W2"].shape == (N1, N2 // 2)
