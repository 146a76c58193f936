"""Running a default-format (QDQ) file with quantized activations on the int8 matrix cores (`GraphRunner(qdq="fused+integer")`) and
scoring it (`onnx_quantize_amd.perplexity(..., qdq="fused+integer")`): routing and counters, the logits beside the default route
by the criteria test_qdq_runner_gpu.py applies to "fused", calls the route leaves to the body, a recorded pass, the perplexity.

The models and configurations are those of test_qdq_runner_gpu.py.  `ops.qdq_function` serves the functions with an input Q -> DQ
(include/oq_hip_qdq_function.h: "no input Q -> DQ" is not a mode of the call): static_in, static_both, dynamic_in, dynamic_both.
The two output-only configurations have no 8-bit activation to multiply; under the new mode they go, and are counted, as under
"fused"."""
import numpy as np
import pytest
import torch

import onnx_quantize_amd as oq
from onnx_quantize_amd import onnx_proto as P
from onnx_quantize_amd.graph_runner import GraphRunner
from test_evaluate_gpu import LENGTH, restated_perplexity
from test_qdq_runner_gpu import CONFIGS, MODELS, Restated, call_of, copy_of, feed_of, levels_apart, quantized

pytestmark = pytest.mark.gpu

INTEGER = ["static_in", "static_both", "dynamic_in", "dynamic_both"]
OUTPUT_ONLY = ["static_out", "dynamic_out"]


@pytest.fixture(scope="module")
def tokens():
    from test_evaluate_gpu import VOCAB
    return np.random.default_rng(1).integers(0, VOCAB, LENGTH)


@pytest.mark.parametrize("config", INTEGER)
@pytest.mark.parametrize("which", sorted(MODELS))
def test_the_integer_route_takes_the_call_and_its_logits_hold(which, config, tokens):
    model, feed = quantized(which, config), feed_of(which, tokens)
    integer, default = GraphRunner(model, device="cuda", qdq="fused+integer"), GraphRunner(model, device="cuda")
    a, b = integer(feed)["logits"], default(feed)["logits"]
    assert integer.qdq == "fused+integer"
    assert integer.qdq_function_calls == {"integer": 1, "body": 0} and integer.qdq_calls == {"fused": 0, "torch": 0}
    assert default.qdq_function_calls == {"integer": 0, "body": 0} and default.qdq_calls == {"fused": 0, "torch": 1}
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape
    _, act_in, act_out, _ = CONFIGS[config]
    if act_out is None:
        # Against float64 of the file's integers and the default route's x_dequantized.  The integer route: four roundings of v
        # (include/oq_hip_qdq_function.h, `error`) and the one of x_dequantized itself, which float64 carries and the integer sum does
        # not: 5 * 2^-24 of the magnitude.  The default route: an fp32 GEMM on the rounded dequantized weight, inside `Case.bound`.
        c = Restated(model, default, feed)
        y64, mine = c.y64(), 5 * 2.0 ** -24 * (1 + 2.0 ** -20) * c.magnitude()
        excess = ((a.reshape(-1, c.N).double() - y64).abs() - mine).max().item()
        between = ((a.double() - b.double()).reshape(-1, c.N).abs() - (mine + c.bound())).max().item()
        print(f"{which} {config}: max(|err| - bound) = {excess:.3e}, beside the default route {between:.3e}, |Y64| up to {float(y64.abs().max()):.3g}")
        assert excess <= 0.0 and between <= 0.0 and float(y64.abs().max()) > 1.0
    elif act_out.is_static:
        _, _, names = call_of(model)
        step = float(P.tensor_to_numpy(next(t for t in model.graph.initializer if t.name == names["out_scale"])))
        apart = levels_apart(a, b, step)
        print(f"{which} {config}: out_scale {step:.4g}, at most {apart:.4g} levels apart")
        assert apart <= 1 + 2.0 ** -20
        assert float(b.abs().max()) > 20 * step
    else:
        step = float(torch.clamp(b.max(), min=0.0) - torch.clamp(b.min(), max=0.0)) / 255
        apart = levels_apart(a, b, step)
        print(f"{which} {config}: level {step:.4g}, at most {apart:.4g} levels apart")
        assert apart <= 2.01


@pytest.mark.parametrize("config", OUTPUT_ONLY + ["default", "channel", "int4_g32"])
@pytest.mark.parametrize("which", sorted(MODELS))
def test_every_other_file_gives_the_bytes_and_counts_of_fused(which, config, tokens):
    model, feed = quantized(which, config), feed_of(which, tokens)
    integer, fused = GraphRunner(model, device="cuda", qdq="fused+integer"), GraphRunner(model, device="cuda", qdq="fused")
    a, b = integer(feed)["logits"], fused(feed)["logits"]
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert integer.qdq_calls == fused.qdq_calls == {"fused": 1, "torch": 0}
    assert integer.qdq_function_calls == fused.qdq_function_calls == {"integer": 0, "body": 0}


def walks_the_body(model, feed):
    integer, default = GraphRunner(model, device="cuda", qdq="fused+integer"), GraphRunner(model, device="cuda")
    a, b = integer(feed)["logits"], default(feed)["logits"]
    assert integer.qdq_function_calls == {"integer": 0, "body": 1} and integer.qdq_calls == {"fused": 0, "torch": 0}
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_an_edited_body_walks_the_body(tokens):
    model = copy_of(quantized("matmul", "static_in"))
    _, fn, _ = call_of(model)
    fn.node[0].attribute = list(fn.node[0].attribute) + [P.make_attribute("axis", 1)]
    walks_the_body(model, feed_of("matmul", tokens))


def test_a_scale_fed_as_a_graph_input_walks_the_body(tokens):
    model = copy_of(quantized("matmul", "static_in"))
    _, _, names = call_of(model)
    s = next(t for t in model.graph.initializer if t.name == names["x_scale"])
    model.graph.initializer = [t for t in model.graph.initializer if t.name != s.name]
    model.graph.input = list(model.graph.input) + [P.make_value_info(s.name, s.data_type, list(s.dims))]
    walks_the_body(model, {"input_ids": feed_of("matmul", tokens), s.name: torch.from_numpy(P.tensor_to_numpy(s).copy())})


def test_an_fp16_activation_walks_the_body(tokens):
    """The embedding table as fp16: X reaches the function as fp16, which the call refuses by name."""
    model = copy_of(quantized("matmul", "dynamic_in"))
    node, _, _ = call_of(model)
    gather = next(n for n in model.graph.node if node.input[0] in n.output)
    table = next(t for t in model.graph.initializer if t.name == gather.input[0])
    half = P.numpy_to_tensor(table.name, P.tensor_to_numpy(table).astype(np.float16))
    model.graph.initializer = [half if t.name == table.name else t for t in model.graph.initializer]
    walks_the_body(model, feed_of("matmul", tokens))


@pytest.mark.parametrize("config", ["static_both", "dynamic_both"])
def test_an_integer_pass_is_recordable(config, tokens):
    model, feed = quantized("matmul", config), feed_of("matmul", tokens)
    eager = GraphRunner(model, device="cuda", qdq="fused+integer")
    rec = GraphRunner(model, device="cuda", qdq="fused+integer", capture=True)
    for i in range(4):
        assert torch.equal(eager(feed)["logits"].view(torch.uint8), rec(feed)["logits"].view(torch.uint8)), i
    assert next(iter(rec._graphs.values())) is not None, "a pass on the integer route synchronises with nothing: it can be recorded"
    assert rec.qdq_function_calls["body"] == 0 and rec.qdq_function_calls["integer"] >= 1


@pytest.mark.parametrize("config", ["static_in", "dynamic_both"])
def test_perplexity_equals_the_restated_loop(tokens, config):
    model = quantized("matmul", config)
    want, count = restated_perplexity(GraphRunner(model, device="cuda", qdq="fused+integer"), tokens, 16, 5)
    got = oq.perplexity(model, tokens, max_length=16, stride=5, qdq="fused+integer")
    assert count == LENGTH - 1
    assert abs(got - want) <= 1e-9 * want, (got, want)
    assert np.isfinite(got) and got > 1.0


def test_other_values_of_the_option_are_still_refused_and_a_cpu_runner_stays_on_torch():
    model = quantized("matmul", "static_in")
    with pytest.raises(ValueError, match="qdq"):
        GraphRunner(model, device="cuda", qdq="hip")
    with pytest.raises(ValueError, match="qdq"):
        oq.perplexity(model, np.arange(8), qdq="hip")
    assert GraphRunner(model, device="cpu", qdq="fused+integer").qdq == "torch"
    assert GraphRunner.evaluator(21).qdq_function_calls == {"integer": 0, "body": 0}
