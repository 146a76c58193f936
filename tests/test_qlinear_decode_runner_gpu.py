"""`GraphRunner(qlinear="fused+decode")` and `onnx_quantize_amd.perplexity(..., qlinear="fused+decode")`: a QLinearMatMul / QGemm node
whose flattened A has at most 16 rows runs on the decode kernel (`ops.qlinear_matmul_decode`) and is counted as "decode"; the
accumulator and the epilogue are those of the tile kernel, so the logits have the bytes of the "fused" runner's.

The models are those of test_qlinear_runner_gpu.py: the tiny LM (Gather -> MatMul) and its Gemm twin, quantized the same way."""
import numpy as np
import pytest
import torch

import onnx_quantize_amd as oq
from onnx_quantize_amd import quantize
from onnx_quantize_amd.graph_runner import GraphRunner
from test_evaluate_gpu import LENGTH, VOCAB, tiny_lm
from test_qlinear_runner_gpu import config, gemm_lm, qgemm_model

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


@pytest.mark.parametrize("count", [1, 5, 16])
@pytest.mark.parametrize("which", ["matmul", "gemm"])
def test_feeds_of_at_most_16_tokens_run_on_the_decode_kernel_with_the_bytes_of_the_fused_runner(models, tokens, which, count):
    assert LENGTH >= 17
    feed = feed_of(which, tokens, count)
    decode, fused = GraphRunner(models[which], device="cuda", qlinear="fused+decode"), GraphRunner(models[which], device="cuda", qlinear="fused")
    a, b = decode(feed)["logits"], fused(feed)["logits"]
    assert decode.qlinear == "fused+decode"
    assert decode.qlinear_calls == {"fused": 0, "torch": 0, "decode": 1} and fused.qlinear_calls == {"fused": 1, "torch": 0}
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape and a.shape[-1] == VOCAB
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert len(torch.unique(a)) > 10                                               # the logits do spread over the levels


@pytest.mark.parametrize("which", ["matmul", "gemm"])
def test_17_tokens_stay_on_the_tile_kernel(models, tokens, which):
    feed = feed_of(which, tokens, 17)
    decode, fused = GraphRunner(models[which], device="cuda", qlinear="fused+decode"), GraphRunner(models[which], device="cuda", qlinear="fused")
    a, b = decode(feed)["logits"], fused(feed)["logits"]
    assert decode.qlinear_calls == {"fused": 1, "torch": 0, "decode": 0}
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_the_other_modes_have_no_decode_key_and_other_values_are_refused(models):
    model = models["matmul"]
    assert GraphRunner(model, device="cuda").qlinear_calls == {"fused": 0, "torch": 0}
    assert GraphRunner(model, device="cuda", qlinear="fused").qlinear_calls == {"fused": 0, "torch": 0}
    assert GraphRunner(model, device="cuda", qlinear="fused+decode").qlinear_calls == {"fused": 0, "torch": 0, "decode": 0}
    for value in ("decode", "fused+", "hip"):
        with pytest.raises(ValueError, match="qlinear"):
            GraphRunner(model, device="cuda", qlinear=value)
    cpu = GraphRunner(model, device="cpu", qlinear="fused+decode")
    assert cpu.qlinear == "torch" and cpu.qlinear_calls == {"fused": 0, "torch": 0}   # no kernel runs on the host


def test_a_decode_pass_is_recordable_and_replays_bit_for_bit(models, tokens):
    feed = feed_of("matmul", tokens, 16)
    eager = GraphRunner(models["matmul"], device="cuda", qlinear="fused+decode")
    rec = GraphRunner(models["matmul"], device="cuda", qlinear="fused+decode", capture=True)
    want = eager(feed)["logits"].view(torch.uint8).clone()
    for i in range(4):
        assert torch.equal(rec(feed)["logits"].view(torch.uint8), want), i
    assert next(iter(rec._graphs.values())) is not None, "a pass with the decode kernel synchronises with nothing: it can be recorded"
    assert rec.qlinear_calls["decode"] >= 1 and rec.qlinear_calls["fused"] == 0


@pytest.mark.parametrize("max_length,stride", [(16, 5), (9, 9)])
def test_perplexity_with_windows_of_at_most_16_tokens_equals_the_fused_one(models, tokens, max_length, stride):
    got = oq.perplexity(models["matmul"], tokens, max_length=max_length, stride=stride, qlinear="fused+decode")
    want = oq.perplexity(models["matmul"], tokens, max_length=max_length, stride=stride, qlinear="fused")
    assert got == want and np.isfinite(got) and got > 1.0


def test_a_node_with_alpha_stays_on_the_expansion_route_and_its_twin_without_is_decoded():
    x = torch.from_numpy(np.random.default_rng(11).integers(0, 256, (12, 64)).astype(np.uint8))
    model = qgemm_model(0.5)
    decode, default = GraphRunner(model, device="cuda", qlinear="fused+decode"), GraphRunner(model, device="cuda")
    a, b = decode(x)["Y"], default(x)["Y"]
    assert a.dtype == b.dtype == torch.uint8 and torch.equal(a, b)
    assert decode.qlinear_calls == {"fused": 0, "torch": 1, "decode": 0}
    model = qgemm_model(1.0)
    decode, fused = GraphRunner(model, device="cuda", qlinear="fused+decode"), GraphRunner(model, device="cuda", qlinear="fused")
    a, b = decode(x)["Y"], fused(x)["Y"]
    assert decode.qlinear_calls == {"fused": 0, "torch": 0, "decode": 1} and fused.qlinear_calls == {"fused": 1, "torch": 0}
    assert a.dtype == torch.uint8 and torch.equal(a, b) and len(torch.unique(a)) > 20
