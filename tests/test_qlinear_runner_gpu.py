"""Running a `format="qlinear"` file on the int8 matrix cores (`GraphRunner(qlinear="fused")`) and scoring it
(`onnx_quantize_amd.perplexity(..., qlinear="fused")`): routing and counters, the logits beside the expansion route, a recorded pass,
the perplexity against the NumPy float64 restatement, and a node the kernel leaves out.

The models are the tiny LM of test_evaluate_gpu.py (Gather -> MatMul) and a twin whose head is a Gemm with a bias, quantized here:
int8 symmetric weights, uint8 static activations on both sides, calibrated on random token ids."""
import numpy as np
import pytest
import torch

import onnx_quantize_amd as oq
from onnx_quantize_amd import QActivationArgs, QConfig, QuantType, QWeightArgs, quantize
from onnx_quantize_amd import onnx_proto as P
from onnx_quantize_amd.graph_runner import GraphRunner
from test_evaluate_gpu import LENGTH, VOCAB, WIDTH, restated_perplexity, tiny_lm

pytestmark = pytest.mark.gpu


def config(calibration_data):
    act = QActivationArgs(dtype=QuantType.QUInt8, is_static=True)
    return QConfig(weights=QWeightArgs(dtype=QuantType.QInt8, symmetric=True), format="qlinear", input_activations=act,
                   output_activations=act, calibration_data=calibration_data)


def gemm_lm():
    """input_ids [T] -> Gather(emb) [T, WIDTH] -> Gemm(W [VOCAB, WIDTH], transB = 1, bias) -> logits [T, VOCAB]."""
    rng = np.random.default_rng(3)
    emb = rng.standard_normal((VOCAB, WIDTH)).astype(np.float32)
    w = (rng.standard_normal((VOCAB, WIDTH)) * 0.4).astype(np.float32)
    bias = rng.standard_normal(VOCAB).astype(np.float32)
    nodes = [P.make_node("Gather", ["emb", "input_ids"], ["h"], name="embed", axis=0),
             P.make_node("Gemm", ["h", "W", "bias"], ["logits"], name="lm_head", transB=1)]
    g = P.Message("GraphProto", name="gemm_lm", node=nodes,
                  initializer=[P.numpy_to_tensor("emb", emb), P.numpy_to_tensor("W", w), P.numpy_to_tensor("bias", bias)],
                  input=[P.make_value_info("input_ids", P.DataType.INT64, ["T"])], output=[P.make_value_info("logits", P.DataType.FLOAT, ["T", VOCAB])])
    return P.Message("ModelProto", ir_version=10, graph=g, opset_import=[P.Message("OperatorSetIdProto", domain="", version=21)])


@pytest.fixture(scope="module")
def tokens():
    return np.random.default_rng(1).integers(0, VOCAB, LENGTH)


@pytest.fixture(scope="module")
def quantized():
    data = np.random.default_rng(5).integers(0, VOCAB, (24, 1, 12)).astype(np.int64)
    out = quantize(tiny_lm(), config(data))
    assert [n.op_type for n in out.graph.node if n.domain == "quant"] == ["QLinearMatMul"]
    return out


@pytest.fixture(scope="module")
def quantized_gemm():
    data = np.random.default_rng(5).integers(0, VOCAB, (24 * 12,)).astype(np.int64)
    out = quantize(gemm_lm(), config(data))
    node = next(n for n in out.graph.node if n.domain == "quant")
    assert node.op_type == "QLinearGemm"
    inits = {t.name: t for t in out.graph.initializer}
    assert inits[node.input[2]].data_type == P.DataType.INT32                      # the bias at scale x_scale * w_scale
    return out


def out_scale(model):
    node = next(n for n in model.graph.node if n.domain == "quant")
    fn = next(f for f in model.functions if f.name == node.op_type)
    inits = {t.name: P.tensor_to_numpy(t) for t in model.graph.initializer}
    return float(inits[node.input[list(fn.input).index("out_scale")]])


@pytest.mark.parametrize("which", ["matmul", "gemm"])
def test_the_fused_runner_takes_every_node_and_its_logits_lie_beside_the_expansion_route(quantized, quantized_gemm, tokens, which):
    model = quantized if which == "matmul" else quantized_gemm
    ids = torch.from_numpy(tokens.astype(np.int64))
    feed = ids.reshape(1, -1) if which == "matmul" else ids
    fused, default = GraphRunner(model, device="cuda", qlinear="fused"), GraphRunner(model, device="cuda")
    a, b = fused(feed)["logits"], default(feed)["logits"]
    assert fused.qlinear == "fused" and default.qlinear == "torch"
    assert fused.qlinear_calls == {"fused": 1, "torch": 0} and default.qlinear_calls == {"fused": 0, "torch": 1}
    step = out_scale(model)
    apart = (a.double() - b.double()).abs()
    print(f"{which}: out_scale {step:.4g}, {float((apart != 0).double().mean()):.3%} of the logits differ, by at most {float(apart.max()):.4g}")
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape
    assert float(apart.max()) <= step * (1 + 2.0 ** -20)
    assert float(b.abs().max()) > 20 * step                                        # the logits do spread over the levels


def test_other_values_of_the_option_are_refused_and_a_cpu_runner_stays_on_torch(quantized):
    with pytest.raises(ValueError, match="qlinear"):
        GraphRunner(quantized, device="cuda", qlinear="hip")
    cpu = GraphRunner(quantized, device="cpu", qlinear="fused")
    assert cpu.qlinear == "torch"                                                  # no kernel runs on the host
    assert GraphRunner.evaluator(21).qlinear_calls == {"fused": 0, "torch": 0}


def test_a_fused_pass_is_recordable(quantized, tokens):
    feed = torch.from_numpy(tokens.astype(np.int64)).reshape(1, -1)
    eager = GraphRunner(quantized, device="cuda", qlinear="fused")
    rec = GraphRunner(quantized, device="cuda", qlinear="fused", capture=True)
    for i in range(4):
        assert torch.equal(eager(feed)["logits"].view(torch.uint8), rec(feed)["logits"].view(torch.uint8)), i
    assert next(iter(rec._graphs.values())) is not None, "a pass with the fused kernel synchronises with nothing: it can be recorded"


@pytest.mark.parametrize("max_length,stride", [(16, 5), (64, 512)])
def test_perplexity_equals_the_restated_loop(quantized, tokens, max_length, stride):
    want, count = restated_perplexity(GraphRunner(quantized, device="cuda", qlinear="fused"), tokens, max_length, stride)
    got = oq.perplexity(quantized, tokens, max_length=max_length, stride=stride, qlinear="fused")
    assert count == LENGTH - 1
    assert abs(got - want) <= 1e-9 * want, (got, want)
    assert np.isfinite(got) and got > 1.0
    default = oq.perplexity(quantized, tokens, max_length=max_length, stride=stride)
    want_default, _ = restated_perplexity(GraphRunner(quantized, device="cuda"), tokens, max_length, stride)
    assert abs(default - want_default) <= 1e-9 * want_default                      # the default stays the expansion route


def qgemm_model(alpha):
    """X [M, 64] uint8 -> com.microsoft::QGemm(transB = 1, alpha) -> Y uint8, built by hand."""
    rng = np.random.default_rng(9)
    K, N = 64, 48
    inits = [P.numpy_to_tensor("a_scale", np.float32(0.02)), P.numpy_to_tensor("a_zp", np.uint8(121)),
             P.numpy_to_tensor("B", rng.integers(-128, 128, (N, K)).astype(np.int8)),
             P.numpy_to_tensor("b_scale", (rng.random(N) * 0.004 + 0.008).astype(np.float32)), P.numpy_to_tensor("b_zp", np.zeros(N, np.int8)),
             P.numpy_to_tensor("C", rng.integers(-5000, 5000, N).astype(np.int32)), P.numpy_to_tensor("y_scale", np.float32(0.04)),
             P.numpy_to_tensor("y_zp", np.uint8(128))]
    node = P.make_node("QGemm", ["X", "a_scale", "a_zp", "B", "b_scale", "b_zp", "C", "y_scale", "y_zp"], ["Y"], name="fc", domain="com.microsoft",
                       transB=1, alpha=float(alpha))
    g = P.Message("GraphProto", name="qgemm", node=[node], initializer=inits, input=[P.make_value_info("X", P.DataType.UINT8, ["M", K])],
                  output=[P.make_value_info("Y", P.DataType.UINT8, ["M", N])])
    return P.Message("ModelProto", ir_version=10, graph=g, opset_import=[P.Message("OperatorSetIdProto", domain="", version=21),
                                                                         P.Message("OperatorSetIdProto", domain="com.microsoft", version=1)])


def test_a_node_with_alpha_stays_on_the_expansion_route_and_its_twin_without_is_taken():
    x = torch.from_numpy(np.random.default_rng(11).integers(0, 256, (50, 64)).astype(np.uint8))
    model = qgemm_model(0.5)
    fused, default = GraphRunner(model, device="cuda", qlinear="fused"), GraphRunner(model, device="cuda")
    a, b = fused(x)["Y"], default(x)["Y"]
    assert a.dtype == b.dtype == torch.uint8 and torch.equal(a, b)
    assert fused.qlinear_calls == default.qlinear_calls == {"fused": 0, "torch": 1}
    assert len(torch.unique(b)) > 20
    # the same node with alpha = 1 is taken, and lies beside the expansion by at most one level
    model = qgemm_model(1.0)
    fused, default = GraphRunner(model, device="cuda", qlinear="fused"), GraphRunner(model, device="cuda")
    a, b = fused(x)["Y"], default(x)["Y"]
    assert fused.qlinear_calls == {"fused": 1, "torch": 0}
    assert a.dtype == torch.uint8 and int((a.int() - b.int()).abs().max()) <= 1 and len(torch.unique(b)) > 20
