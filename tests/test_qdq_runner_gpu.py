"""Running a default-format (QDQ) file with its products on the fused kernel (`GraphRunner(qdq="fused")`) and scoring it
(`onnx_quantize_amd.perplexity(..., qdq="fused")`): routing and counters for every function family, the logits against a float64
restatement from the file's initializers (functions without an output Q -> DQ) or beside the default route in output levels
(functions with one), calls the kernel leaves out, a recorded pass, and the perplexity against the NumPy float64 restatement.

The models are the tiny LM of test_evaluate_gpu.py (Gather -> MatMul) and its Gemm twin of test_qlinear_runner_gpu.py, quantized
here.  "default" is the default format with the default weight arguments, `QConfig(weights=QWeightArgs())`: a bare `QConfig()`
selects nothing to quantize and returns the model unchanged."""
import functools

import numpy as np
import pytest
import torch

import nbits_cases
import onnx_quantize_amd as oq
from onnx_quantize_amd import QActivationArgs, QConfig, QuantType, QWeightArgs, quantize
from onnx_quantize_amd import onnx_proto as P
from onnx_quantize_amd.graph_runner import GraphRunner
from test_evaluate_gpu import LENGTH, VOCAB, WIDTH, restated_perplexity, tiny_lm
from test_qlinear_runner_gpu import gemm_lm

pytestmark = pytest.mark.gpu

INT8 = dict(dtype=QuantType.QInt8)
STATIC, DYNAMIC = QActivationArgs(dtype=QuantType.QUInt8, is_static=True), QActivationArgs(dtype=QuantType.QUInt8, is_static=False)
# name -> (weights, input activations, output activations, the function's suffix)
CONFIGS = {
    "default": (QWeightArgs(), None, None, "WeightsOnlyQDQ"),
    "channel": (QWeightArgs(group_size=-1, **INT8), None, None, "WeightsOnlyQDQ"),
    "static_in": (QWeightArgs(**INT8), STATIC, None, None),
    "static_out": (QWeightArgs(**INT8), None, STATIC, None),
    "static_both": (QWeightArgs(**INT8), STATIC, STATIC, None),
    "dynamic_in": (QWeightArgs(**INT8), DYNAMIC, None, "WeightDynamicInputQDQ"),
    "dynamic_out": (QWeightArgs(**INT8), None, DYNAMIC, "WeightDynamicOutputQDQ"),
    "dynamic_both": (QWeightArgs(**INT8), DYNAMIC, DYNAMIC, "WeightDynamicInputOutputQDQ"),
    "int4_g32": (QWeightArgs(dtype=QuantType.QInt4, symmetric=True, group_size=32, strategy="group"), None, None, "WeightsOnlyGrouped"),
}
assert WIDTH % 32 == 0
MODELS = {"matmul": tiny_lm, "gemm": gemm_lm}


def calibration_data(which):
    ids = np.random.default_rng(5).integers(0, VOCAB, (24, 1, 12)).astype(np.int64)
    return ids if which == "matmul" else ids.reshape(-1)


@functools.lru_cache(maxsize=None)
def quantized(which, config):
    weights, act_in, act_out, suffix = CONFIGS[config]
    static = any(a is not None and a.is_static for a in (act_in, act_out))
    out = quantize(MODELS[which](), QConfig(weights=weights, input_activations=act_in, output_activations=act_out,
                                            calibration_data=calibration_data(which) if static else None))
    names = [n.op_type for n in out.graph.node if n.domain == "quant"]
    assert len(names) == 1 and names[0].startswith("QMatMul" if which == "matmul" else "QGemm"), names
    assert suffix is None or names[0].endswith(suffix), names                    # QInt4 group 32 emits ...WeightsOnlyGrouped
    return out


def feed_of(which, tokens):
    ids = torch.from_numpy(tokens.astype(np.int64))
    return ids.reshape(1, -1) if which == "matmul" else ids


@pytest.fixture(scope="module")
def tokens():
    return np.random.default_rng(1).integers(0, VOCAB, LENGTH)


def call_of(model):
    """The quant-domain node, its function, and {function input: the name the call hands in}."""
    node = next(n for n in model.graph.node if n.domain == "quant")
    fn = next(f for f in model.functions if f.name == node.op_type)
    return node, fn, dict(zip(fn.input, node.input))


class Restated(nbits_cases.Case):
    """The float64 product of the file's own initializers with the input side of the default route, judged by `Case.bound`."""

    def __init__(self, model, default, feed):
        node, fn, names = call_of(model)
        inits = {t.name: P.tensor_to_numpy(t) for t in model.graph.initializer}
        w = inits[names["W"]].astype(np.float64)                                                   # [K, N]
        scale, zp = inits[names["w_scale"]].astype(np.float64), inits[names["w_zero_point"]].astype(np.float64)
        K, N = w.shape
        blocks = scale.size // N if scale.size > N else 1
        shape = (1, 1) if scale.size == 1 else (N, blocks)
        w64 = (w.T.reshape(N, blocks, K // blocks) - zp.reshape(shape)[:, :, None]) * scale.reshape(shape)[:, :, None]
        # the input side: the body's own operators in front of the product, run by the default runner
        x = GraphRunner(model, outputs=[node.input[0]], device="cuda")(feed)[node.input[0]]
        env = {name: (x if name == "X" else default.constants[names[name]]) for name in fn.input}
        nodes = list(fn.node)
        product = next(i for i, n in enumerate(nodes) if n.op_type in ("MatMul", "Gemm"))
        with torch.no_grad():
            default._run(nodes[:product], env)
        self.x = env[nodes[product].input[0]].reshape(-1, K)
        self.bias = env[nodes[product].input[2]] if len(nodes[product].input) > 2 else None
        self.w64 = torch.from_numpy(w64.reshape(N, K)).cuda()
        self.M, self.K, self.N, self.group, self.dtype = self.x.shape[0], K, N, K // blocks, self.x.dtype


def levels_apart(a, b, step):
    return float((a.double() - b.double()).abs().max()) / step


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("which", sorted(MODELS))
def test_the_fused_runner_takes_the_call_and_its_logits_hold(which, config, tokens):
    model, feed = quantized(which, config), feed_of(which, tokens)
    fused, default = GraphRunner(model, device="cuda", qdq="fused"), GraphRunner(model, device="cuda")
    a, b = fused(feed)["logits"], default(feed)["logits"]
    assert fused.qdq == "fused" and default.qdq == "torch"
    assert fused.qdq_calls == {"fused": 1, "torch": 0} and default.qdq_calls == {"fused": 0, "torch": 1}
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape
    _, act_in, act_out, _ = CONFIGS[config]
    if act_out is None:                                   # against float64, inside the kernel's bound
        c = Restated(model, default, feed)
        y64 = c.y64()
        excess = ((a.reshape(-1, c.N).double() - y64).abs() - c.bound()).max().item()
        print(f"{which} {config}: max(|err| - bound) = {excess:.3e}, |Y64| up to {float(y64.abs().max()):.3g}")
        assert excess <= 0.0 and float(y64.abs().max()) > 1.0
    elif act_out.is_static:                               # at most one output level from the default route
        node, fn, names = call_of(model)
        step = float(P.tensor_to_numpy(next(t for t in model.graph.initializer if t.name == names["out_scale"])))
        apart = levels_apart(a, b, step)
        print(f"{which} {config}: out_scale {step:.4g}, at most {apart:.4g} levels apart")
        assert apart <= 1 + 2.0 ** -20
        assert float(b.abs().max()) > 20 * step           # the logits do spread over the levels
    else:
        # a level of the default route's dynamic output; one for the value's rounding, one for the zero point's, 1 % for the scale's
        step = float(torch.clamp(b.max(), min=0.0) - torch.clamp(b.min(), max=0.0)) / 255
        apart = levels_apart(a, b, step)
        print(f"{which} {config}: level {step:.4g}, at most {apart:.4g} levels apart")
        assert apart <= 2.01


def test_other_values_of_the_option_are_refused_and_a_cpu_runner_stays_on_torch():
    model = quantized("matmul", "default")
    with pytest.raises(ValueError, match="qdq"):
        GraphRunner(model, device="cuda", qdq="hip")
    assert GraphRunner(model, device="cpu", qdq="fused").qdq == "torch"           # no kernel runs on the host
    assert GraphRunner.evaluator(21).qdq_calls == {"fused": 0, "torch": 0}
    with pytest.raises(ValueError, match="qdq"):
        oq.perplexity(model, np.arange(8), qdq="hip")


def copy_of(model):
    return model.copy()


def stays_on_torch(model, feed):
    fused, default = GraphRunner(model, device="cuda", qdq="fused"), GraphRunner(model, device="cuda")
    a, b = fused(feed)["logits"], default(feed)["logits"]
    assert fused.qdq_calls == default.qdq_calls == {"fused": 0, "torch": 1}
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_an_edited_body_under_the_reference_name_stays_on_the_function_body(tokens):
    """The same arithmetic, another body: the weight's DequantizeLinear names its (default) axis.  Recognition compares the body."""
    model = copy_of(quantized("matmul", "default"))
    _, fn, _ = call_of(model)
    fn.node[0].attribute = list(fn.node[0].attribute) + [P.make_attribute("axis", 1)]
    stays_on_torch(model, feed_of("matmul", tokens))
    model = copy_of(quantized("matmul", "default"))                              # and other wiring: an Identity in front of the product
    _, fn, _ = call_of(model)
    fn.node = [fn.node[0], P.make_node("Identity", ["dequantized_weights"], ["w2"]), P.make_node("MatMul", ["X", "w2"], ["out"])]
    stays_on_torch(model, feed_of("matmul", tokens))


def test_a_group_size_of_16_stays_on_the_function_body(tokens):
    model = quantize(tiny_lm(), QConfig(weights=QWeightArgs(dtype=QuantType.QInt4, symmetric=True, group_size=16, strategy="group")))
    assert [n.op_type for n in model.graph.node if n.domain == "quant"] == ["QMatMulWeightsOnlyGrouped"]
    stays_on_torch(model, feed_of("matmul", tokens))


def test_a_weight_fed_as_a_graph_input_stays_on_the_function_body(tokens):
    model = copy_of(quantized("matmul", "default"))
    _, _, names = call_of(model)
    w = next(t for t in model.graph.initializer if t.name == names["W"])
    model.graph.initializer = [t for t in model.graph.initializer if t.name != w.name]
    model.graph.input = list(model.graph.input) + [P.make_value_info(w.name, w.data_type, list(w.dims))]
    feed = {"input_ids": feed_of("matmul", tokens), w.name: torch.from_numpy(P.tensor_to_numpy(w).copy())}
    stays_on_torch(model, feed)


@pytest.mark.parametrize("config", ["default", "static_both", "int4_g32"])
def test_a_fused_pass_is_recordable(config, tokens):
    model, feed = quantized("matmul", config), feed_of("matmul", tokens)
    eager = GraphRunner(model, device="cuda", qdq="fused")
    rec = GraphRunner(model, device="cuda", qdq="fused", capture=True)
    for i in range(4):
        assert torch.equal(eager(feed)["logits"].view(torch.uint8), rec(feed)["logits"].view(torch.uint8)), i
    assert next(iter(rec._graphs.values())) is not None, "a pass with the fused kernel synchronises with nothing: it can be recorded"
    assert rec.qdq_calls["torch"] == 0


@pytest.mark.parametrize("max_length,stride", [(16, 5), (64, 512)])
def test_perplexity_equals_the_restated_loop(tokens, max_length, stride):
    model = quantized("matmul", "default")
    want, count = restated_perplexity(GraphRunner(model, device="cuda", qdq="fused"), tokens, max_length, stride)
    got = oq.perplexity(model, tokens, max_length=max_length, stride=stride, qdq="fused")
    assert count == LENGTH - 1
    assert abs(got - want) <= 1e-9 * want, (got, want)
    assert np.isfinite(got) and got > 1.0
    default = oq.perplexity(model, tokens, max_length=max_length, stride=stride)
    want_default, _ = restated_perplexity(GraphRunner(model, device="cuda"), tokens, max_length, stride)
    assert abs(default - want_default) <= 1e-9 * want_default                    # the default stays the function body
