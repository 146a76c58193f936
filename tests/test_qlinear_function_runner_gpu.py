"""`GraphRunner(qlinear="function")` / `"function+decode"` and `onnx_quantize_amd.perplexity(..., qlinear=...)`: a call of a
`quant`-domain QLinearMatMul / QLinearGemm function whose body is the writer's runs as ONE library call (`ops.qlinear_function`; at
most 16 flattened rows: `ops.qlinear_function_decode`) and is counted in `qlinear_function_calls`; every other call walks its body,
whose integer node goes as under "fused" / "fused+decode".  The logits have the bytes of the "fused" runner's.

The models are those of test_qlinear_decode_runner_gpu.py: the tiny LM (Gather -> MatMul) and its Gemm twin, quantized the same way."""
import numpy as np
import pytest
import torch

import onnx_quantize_amd as oq
from onnx_quantize_amd import onnx_proto as P
from onnx_quantize_amd import quantize
from onnx_quantize_amd.graph_runner import GraphRunner
from test_evaluate_gpu import LENGTH, VOCAB, tiny_lm
from test_qlinear_runner_gpu import config, gemm_lm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tokens():
    return np.random.default_rng(1).integers(0, VOCAB, LENGTH)


@pytest.fixture(scope="module")
def models():
    matmul = quantize(tiny_lm(), config(np.random.default_rng(5).integers(0, VOCAB, (24, 1, 12)).astype(np.int64)))
    gemm = quantize(gemm_lm(), config(np.random.default_rng(5).integers(0, VOCAB, (24 * 12,)).astype(np.int64)))
    assert [n.op_type for n in matmul.graph.node if n.domain == "quant"] == ["QLinearMatMul"]
    assert [n.op_type for n in gemm.graph.node if n.domain == "quant"] == ["QLinearGemm"]
    return {"matmul": matmul, "gemm": gemm}


def feed_of(which, tokens, count):
    ids = torch.from_numpy(tokens[:count].astype(np.int64))
    return ids.reshape(1, -1) if which == "matmul" else ids


def same_bytes(a, b):
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("count", [17, LENGTH])
@pytest.mark.parametrize("which", ["matmul", "gemm"])
def test_a_function_call_is_one_library_call_with_the_bytes_of_the_fused_runner(models, tokens, which, count):
    assert LENGTH > 17
    feed = feed_of(which, tokens, count)
    one, fused = GraphRunner(models[which], device="cuda", qlinear="function"), GraphRunner(models[which], device="cuda", qlinear="fused")
    a, b = one(feed)["logits"], fused(feed)["logits"]
    assert one.qlinear == "function"
    assert one.qlinear_function_calls == {"function": 1, "body": 0} and one.qlinear_calls == {"fused": 0, "torch": 0}
    assert fused.qlinear_calls == {"fused": 1, "torch": 0} and fused.qlinear_function_calls == {"function": 0, "body": 0}
    assert same_bytes(a, b) and a.shape[-1] == VOCAB
    assert len(torch.unique(a)) > 10                                               # the logits do spread over the levels


@pytest.mark.parametrize("count", [1, 5, 16])
@pytest.mark.parametrize("which", ["matmul", "gemm"])
def test_feeds_of_at_most_16_tokens_run_on_the_decode_entry_point(models, tokens, which, count):
    feed = feed_of(which, tokens, count)
    one, fused = GraphRunner(models[which], device="cuda", qlinear="function+decode"), GraphRunner(models[which], device="cuda", qlinear="fused")
    a, b = one(feed)["logits"], fused(feed)["logits"]
    assert one.qlinear_function_calls == {"function": 0, "decode": 1, "body": 0} and one.qlinear_calls == {"fused": 0, "torch": 0, "decode": 0}
    assert same_bytes(a, b)


@pytest.mark.parametrize("which", ["matmul", "gemm"])
def test_17_tokens_go_to_the_tile_entry_point(models, tokens, which):
    feed = feed_of(which, tokens, 17)
    one, fused = GraphRunner(models[which], device="cuda", qlinear="function+decode"), GraphRunner(models[which], device="cuda", qlinear="fused")
    a, b = one(feed)["logits"], fused(feed)["logits"]
    assert one.qlinear_function_calls == {"function": 1, "decode": 0, "body": 0}
    assert same_bytes(a, b)


def with_identity_in_the_body(model):
    """The model with an Identity between the integer node and the DequantizeLinear of its QLinear function: the same values, another body."""
    model = model.copy()
    fn = next(f for f in model.functions if f.name in ("QLinearMatMul", "QLinearGemm"))
    q, core, dq = list(fn.node)
    assert dq.op_type == "DequantizeLinear" and dq.input[0] == "out"
    fn.node = [q, core, P.make_node("Identity", ["out"], ["out_again"]),
               P.make_node("DequantizeLinear", ["out_again"] + list(dq.input[1:]), list(dq.output))]
    return model


@pytest.mark.parametrize("mode,count,route", [("function", 17, "fused"), ("function+decode", 5, "decode")])
@pytest.mark.parametrize("which", ["matmul", "gemm"])
def test_a_function_with_another_body_under_the_reference_name_runs_its_body(models, tokens, which, mode, count, route):
    feed = feed_of(which, tokens, count)
    other = GraphRunner(with_identity_in_the_body(models[which]), device="cuda", qlinear=mode)
    fused = GraphRunner(models[which], device="cuda", qlinear="fused")
    a, b = other(feed)["logits"], fused(feed)["logits"]
    want = {"function": 0, "body": 1, **({"decode": 0} if mode == "function+decode" else {})}
    assert other.qlinear_function_calls == want
    assert other.qlinear_calls[route] == 1 and sum(other.qlinear_calls.values()) == 1      # the body's integer node took the kernel
    assert same_bytes(a, b)


def test_a_call_whose_x_scale_is_a_graph_input_runs_its_body(models, tokens):
    model = models["matmul"].copy()
    node = next(n for n in model.graph.node if n.domain == "quant")
    fn = next(f for f in model.functions if f.name == node.op_type)
    name = node.input[list(fn.input).index("x_scale")]
    value = next(P.tensor_to_numpy(t) for t in model.graph.initializer if t.name == name)
    model.graph.initializer = [t for t in model.graph.initializer if t.name != name]
    model.graph.input = list(model.graph.input) + [P.make_value_info(name, P.DataType.FLOAT, [])]
    ids = feed_of("matmul", tokens, 17)
    feed = {"input_ids": ids, name: torch.from_numpy(np.asarray(value, np.float32))}
    one = GraphRunner(model, device="cuda", qlinear="function")
    a = one(feed)["logits"]
    b = GraphRunner(models["matmul"], device="cuda", qlinear="fused")(ids)["logits"]
    assert one.qlinear_function_calls == {"function": 0, "body": 1} and one.qlinear_calls == {"fused": 1, "torch": 0}
    assert same_bytes(a, b)


@pytest.mark.parametrize("mode,count", [("function", LENGTH), ("function+decode", 16)])
def test_a_recorded_pass_replays_bit_for_bit(models, tokens, mode, count):
    feed = feed_of("matmul", tokens, count)
    eager = GraphRunner(models["matmul"], device="cuda", qlinear=mode)
    rec = GraphRunner(models["matmul"], device="cuda", qlinear=mode, capture=True)
    want = eager(feed)["logits"].view(torch.uint8).clone()
    for i in range(4):
        assert torch.equal(rec(feed)["logits"].view(torch.uint8), want), i
    assert next(iter(rec._graphs.values())) is not None, "a pass with the function kernels synchronises with nothing: it can be recorded"
    assert rec.qlinear_function_calls["body"] == 0 and rec.qlinear_function_calls["decode" if mode == "function+decode" else "function"] >= 1


@pytest.mark.parametrize("mode", ["function", "function+decode"])
@pytest.mark.parametrize("max_length,stride", [(16, 5), (9, 9), (LENGTH, LENGTH)])
def test_perplexity_equals_the_fused_one(models, tokens, mode, max_length, stride):
    got = oq.perplexity(models["matmul"], tokens, max_length=max_length, stride=stride, qlinear=mode)
    want = oq.perplexity(models["matmul"], tokens, max_length=max_length, stride=stride, qlinear="fused")
    assert got == want and np.isfinite(got) and got > 1.0


def test_counters_per_mode_refusals_and_a_cpu_runner(models):
    model = models["matmul"]
    assert GraphRunner(model, device="cuda", qlinear="function").qlinear_function_calls == {"function": 0, "body": 0}
    assert GraphRunner(model, device="cuda", qlinear="function").qlinear_calls == {"fused": 0, "torch": 0}
    assert GraphRunner(model, device="cuda", qlinear="function+decode").qlinear_function_calls == {"function": 0, "decode": 0, "body": 0}
    assert GraphRunner(model, device="cuda", qlinear="function+decode").qlinear_calls == {"fused": 0, "torch": 0, "decode": 0}
    for value in ("decode", "fused+", "hip", "function+", "function+fused", "Function"):
        with pytest.raises(ValueError, match="qlinear"):
            GraphRunner(model, device="cuda", qlinear=value)
    cpu = GraphRunner(model, device="cpu", qlinear="function+decode")
    assert cpu.qlinear == "torch" and cpu.qlinear_calls == {"fused": 0, "torch": 0}   # no kernel runs on the host
    assert cpu.qlinear_function_calls == {"function": 0, "body": 0}
