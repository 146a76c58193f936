"""Running a quantized file on the fused MatMulNBits kernel (`GraphRunner(matmul_nbits="fused")`) and scoring it
(`onnx_quantize_amd.perplexity`): routing and counters, the logits against the float64 dequantized product, the windows of the
sliding-window perplexity against a NumPy float64 restatement, and the fused route against the expansion route.

The model is built here from `onnx_proto` messages: a tiny LM, Gather(emb [64, 64], input_ids) -> MatMul(W [64, 64]) -> logits,
|logits| around 10 or less, quantized here at uint4, group size 32."""
import numpy as np
import pytest
import torch

import onnx_quantize_amd as oq
from onnx_quantize_amd import HqqConfig, QConfig, QuantType, QWeightArgs, quantize
from onnx_quantize_amd import onnx_proto as P
from onnx_quantize_amd.evaluate import perplexity_windows
from onnx_quantize_amd.graph_runner import GraphRunner

pytestmark = pytest.mark.gpu

VOCAB, WIDTH, LENGTH = 64, 64, 50


def tiny_lm(extra_input=None):
    rng = np.random.default_rng(0)
    emb = rng.standard_normal((VOCAB, WIDTH)).astype(np.float32)
    w = (rng.standard_normal((WIDTH, VOCAB)) * 0.4).astype(np.float32)
    nodes = [P.make_node("Gather", ["emb", "input_ids"], ["h"], name="embed", axis=0),
             P.make_node("MatMul", ["h", "W"], ["logits"], name="lm_head")]
    inputs = [P.make_value_info("input_ids", P.DataType.INT64, [1, "T"])]
    if extra_input:
        inputs.append(P.make_value_info(extra_input, P.DataType.INT64, [1, "T"]))
    g = P.Message("GraphProto", name="tiny_lm", node=nodes, initializer=[P.numpy_to_tensor("emb", emb), P.numpy_to_tensor("W", w)],
                  input=inputs, output=[P.make_value_info("logits", P.DataType.FLOAT, [1, "T", VOCAB])])
    return P.Message("ModelProto", ir_version=10, graph=g, opset_import=[P.Message("OperatorSetIdProto", domain="", version=21)])


@pytest.fixture(scope="module")
def quantized():
    out = quantize(tiny_lm(), QConfig(weights=QWeightArgs(dtype=QuantType.QUInt4, group_size=32, strategy="group")))
    assert "MatMulNBits" in [n.op_type for n in out.graph.node]
    return out


@pytest.fixture(scope="module")
def hqq_file():
    out = quantize(tiny_lm(), QConfig(weights=QWeightArgs(dtype=QuantType.QUInt4, group_size=32, strategy="group", algorithm=HqqConfig())))
    node = next(n for n in out.graph.node if n.op_type == "MatMulNBits")
    inits = {t.name: t for t in out.graph.initializer}
    assert inits[node.input[3]].data_type == P.DataType.FLOAT                     # float zero points
    return out


@pytest.fixture(scope="module")
def tokens():
    return np.random.default_rng(1).integers(0, VOCAB, LENGTH)


def test_the_fused_runner_takes_the_node_and_its_logits_hold_the_kernel_bound(quantized, tokens):
    node = next(n for n in quantized.graph.node if n.op_type == "MatMulNBits")
    feed = torch.from_numpy(tokens.astype(np.int64)).reshape(1, -1)
    runner = GraphRunner(quantized, outputs=[node.input[0], "logits"], device="cuda", matmul_nbits="fused")
    got = runner(feed)
    assert runner.nbits_calls["fused"] >= 1 and runner.nbits_calls["torch"] == 0
    default = GraphRunner(quantized, device="cuda")
    default(feed)
    assert default.nbits_calls == {"fused": 0, "torch": 1}
    # the float64 dequantized product of the file's own initializers
    inits = {t.name: P.tensor_to_numpy(t) for t in quantized.graph.initializer}
    attrs = {a.name: P.attribute_value(a) for a in node.attribute}
    K, N, g = attrs["K"], attrs["N"], attrs["block_size"]
    blocks = K // g
    blob = inits[node.input[1]].reshape(N, blocks, g // 2)
    q = np.stack([blob & 0xF, blob >> 4], axis=-1).reshape(N, blocks, g).astype(np.float64)
    zb = inits[node.input[3]].reshape(N, -1)
    zp = np.stack([zb & 0xF, zb >> 4], axis=-1).reshape(N, -1)[:, :blocks].astype(np.float64)
    w64 = ((q - zp[:, :, None]) * inits[node.input[2]].reshape(N, blocks, 1).astype(np.float64)).reshape(N, K)
    a64 = got[node.input[0]].reshape(-1, K).double().cpu().numpy()
    y64 = a64 @ w64.T
    s = np.abs(a64) @ np.abs(w64).T
    term = (K + 2 * blocks + 4) * 2.0 ** -23 * s + 2.0 ** -21 * s + K * 2.0 ** -38 * np.abs(a64).max(axis=1, keepdims=True) * np.abs(w64).max()
    bound = term + 2.0 ** -24 * (np.abs(y64) + term)
    err = np.abs(got["logits"].reshape(-1, N).double().cpu().numpy() - y64)
    assert np.abs(y64).max() < 20 and (err <= bound).all(), (err - bound).max()


def test_float_zero_points_stay_on_the_expansion_route(hqq_file, tokens):
    feed = torch.from_numpy(tokens.astype(np.int64)).reshape(1, -1)
    fused, default = GraphRunner(hqq_file, device="cuda", matmul_nbits="fused"), GraphRunner(hqq_file, device="cuda")
    a, b = fused(feed)["logits"], default(feed)["logits"]
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert fused.nbits_calls == {"fused": 0, "torch": 1}


def test_other_values_of_the_option_are_refused(quantized):
    with pytest.raises(ValueError, match="matmul_nbits"):
        GraphRunner(quantized, device="cuda", matmul_nbits="hip")
    assert GraphRunner(quantized, device="cpu", matmul_nbits="fused").matmul_nbits == "torch"      # no kernel runs on the host


def test_a_fused_pass_is_recordable(quantized, tokens):
    feed = torch.from_numpy(tokens.astype(np.int64)).reshape(1, -1)
    eager = GraphRunner(quantized, device="cuda", matmul_nbits="fused")
    rec = GraphRunner(quantized, device="cuda", matmul_nbits="fused", capture=True)
    for i in range(4):
        assert torch.equal(eager(feed)["logits"], rec(feed)["logits"]), i
    assert next(iter(rec._graphs.values())) is not None, "a pass with the fused kernel synchronises with nothing: it can be recorded"


def restated_perplexity(runner, ids, max_length, stride):
    """The loop of the reference's tools/perplexity.py in NumPy float64, on the logits `runner` returns per window."""
    total, count, prev_end = 0.0, 0, 0
    for begin in range(0, len(ids), stride):
        end = min(begin + max_length, len(ids))
        new = end - prev_end
        chunk = ids[begin:end].astype(np.int64)
        logits = runner(torch.from_numpy(chunk[None, :]))["logits"][0].double().cpu().numpy()
        x = logits[:-1] - logits[:-1].max(axis=-1, keepdims=True)
        log_probs = x - np.log(np.exp(x).sum(axis=-1, keepdims=True))
        targets = chunk[1:][-new:]
        picked = log_probs[-new:][np.arange(len(targets)), targets]
        total, count, prev_end = total - picked.sum(), count + len(picked), end
        if end == len(ids):
            break
    return float(np.exp(total / count)), count


@pytest.mark.parametrize("max_length,stride,counted", [(16, 5, LENGTH - 1), (16, 16, LENGTH - 4), (64, 512, LENGTH - 1)])
def test_perplexity_equals_the_restated_loop(quantized, tokens, max_length, stride, counted):
    """Both sides float64: only the order of the sum differs.  Every token but the first is a counted target (LENGTH - 1) wherever
    a window sees the token in front of its first new target -- overlapping windows, or one window.  With stride == max_length the
    windows do not overlap, and the reference's loop (`targets[-trg_len:]` of a window's n - 1 targets) then scores n - 1 targets
    per window: the first token of each of the four windows has no prediction, LENGTH - 4 are counted.  That is the reference's
    count and so this package's."""
    want, count = restated_perplexity(GraphRunner(quantized, device="cuda", matmul_nbits="fused"), tokens, max_length, stride)
    got = oq.perplexity(quantized, tokens, max_length=max_length, stride=stride)
    assert count == counted == sum(c for _, _, c in perplexity_windows(LENGTH, max_length, stride))
    assert abs(got - want) <= 1e-9 * want, (got, want)
    assert np.isfinite(got) and got > 1.0
    assert oq.perplexity(P.serialize(quantized), tokens, max_length=max_length, stride=stride) == got        # bytes: the same model


def test_inputs_nobody_feeds_and_feeds_nobody_declared_raise_by_name(quantized, tokens):
    with pytest.raises(ValueError, match="'past_keys'"):
        oq.perplexity(quantized, tokens, max_length=16, stride=5, extra_feeds={"past_keys": np.zeros((1, 0), np.float32)})
    with_mask = tiny_lm(extra_input="attention_mask")                             # declared and known: fed with ones
    assert oq.perplexity(with_mask, tokens, max_length=16, stride=5) > 1.0
    with_extra = tiny_lm(extra_input="segment_ids")
    with pytest.raises(ValueError, match="'segment_ids'"):
        oq.perplexity(with_extra, tokens, max_length=16, stride=5)
    seen = []

    def extra(n):
        seen.append(n)
        return {"segment_ids": np.zeros((1, n), np.int64)}

    assert oq.perplexity(with_extra, tokens, max_length=16, stride=16, extra_feeds=extra) > 1.0
    assert seen == [16, 16, 16, 2]
    with pytest.raises(ValueError, match="1-D"):
        oq.perplexity(quantized, tokens.reshape(2, -1))


def test_the_fused_route_scores_within_twice_the_logit_distance_of_the_expansion_route(quantized, tokens):
    """log-softmax moves by at most twice the sup-norm change of its input, and the mean NLL is an average of its entries."""
    feed = torch.from_numpy(tokens.astype(np.int64)).reshape(1, -1)
    # the windows below see the prefixes of `tokens`, and this model scores every position on its own: one pass covers their logits
    fused = GraphRunner(quantized, device="cuda", matmul_nbits="fused")(feed)["logits"].double()
    plain = GraphRunner(quantized, device="cuda")(feed)["logits"].double()
    distance = (fused - plain).abs().max().item()
    a = oq.perplexity(quantized, tokens, max_length=64, stride=512, matmul_nbits="fused")
    b = oq.perplexity(quantized, tokens, max_length=64, stride=512, matmul_nbits="torch")
    assert abs(np.log(a) - np.log(b)) <= 2 * distance, (a, b, distance)
    assert distance < 1e-3


# ------------------------------------------------------------------------------------ routing of nodes the writer here does not emit
def one_node_model(bits, block_size, bias_dtype=None, K=128, N=48):
    """X [M, K] fp32 -> MatMulNBits -> Y, built by hand: q, integer zero points and scales drawn here, a bias of `bias_dtype`."""
    rng = np.random.default_rng(bits * 1000 + block_size)
    blocks = K // block_size
    q = rng.integers(0, 1 << bits, (N, blocks, block_size)).astype(np.uint8)
    zp = rng.integers(0, 1 << bits, (N, blocks)).astype(np.uint8)
    scales = (rng.random((N, blocks)) * 0.02 + 0.001).astype(np.float32)
    if bits == 4:
        blob, zp_stored = q[..., 0::2] | (q[..., 1::2] << 4), zp[:, 0::2] | (zp[:, 1::2] << 4)
    else:
        blob, zp_stored = q, zp
    inits = [P.numpy_to_tensor("B", blob), P.numpy_to_tensor("S", scales), P.numpy_to_tensor("Z", zp_stored)]
    names = ["X", "B", "S", "Z"]
    if bias_dtype is not None:
        inits.append(P.numpy_to_tensor("bias", rng.standard_normal(N).astype(bias_dtype)))
        names += [None, "bias"]
    node = P.make_node("MatMulNBits", names, ["Y"], name="fc", domain="com.microsoft", K=K, N=N, bits=bits, block_size=block_size)
    g = P.Message("GraphProto", name="one_node", node=[node], initializer=inits, input=[P.make_value_info("X", P.DataType.FLOAT, ["M", K])],
                  output=[P.make_value_info("Y", P.DataType.FLOAT, ["M", N])])
    model = P.Message("ModelProto", ir_version=10, graph=g, opset_import=[P.Message("OperatorSetIdProto", domain="", version=21),
                                                                          P.Message("OperatorSetIdProto", domain="com.microsoft", version=1)])
    return model


@pytest.fixture(scope="module")
def rows():
    return torch.from_numpy(np.random.default_rng(7).standard_normal((50, 128)).astype(np.float32))


def test_an_8_bit_node_of_group_64_takes_the_fused_route_and_holds_the_kernel_bound(rows):
    model = one_node_model(8, 64, np.float32)
    runner = GraphRunner(model, device="cuda", matmul_nbits="fused")
    got = runner(rows)["Y"]
    assert runner.nbits_calls == {"fused": 1, "torch": 0}
    # the float64 dequantized product of the file's own initializers
    inits = {t.name: P.tensor_to_numpy(t) for t in P.parse_model(P.serialize(model)).graph.initializer}
    K, N, blocks = 128, 48, 2
    w64 = ((inits["B"].reshape(N, blocks, 64).astype(np.float64) - inits["Z"].reshape(N, blocks, 1)) * inits["S"].reshape(N, blocks, 1).astype(np.float64)).reshape(N, K)
    bias64 = inits["bias"].astype(np.float64)
    a64 = rows.double().numpy()
    y64 = a64 @ w64.T + bias64
    s = np.abs(a64) @ np.abs(w64).T + np.abs(bias64)
    term = (K + 2 * blocks + 4) * 2.0 ** -23 * s + 2.0 ** -21 * s + K * 2.0 ** -38 * np.abs(a64).max(axis=1, keepdims=True) * np.abs(w64).max()
    bound = term + 2.0 ** -24 * (np.abs(y64) + term)
    err = np.abs(got.double().cpu().numpy() - y64)
    assert got.dtype == torch.float32 and (err <= bound).all(), (err - bound).max()


@pytest.mark.parametrize("what", ["block_size = 16", "a bias of another element type than A"])
def test_nodes_the_kernel_leaves_out_stay_on_the_expansion_route(rows, what):
    model = one_node_model(4, 16, np.float32) if what == "block_size = 16" else one_node_model(4, 32, np.float16)
    fused, default = GraphRunner(model, device="cuda", matmul_nbits="fused"), GraphRunner(model, device="cuda")
    a, b = fused(rows)["Y"], default(rows)["Y"]
    assert a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert fused.nbits_calls == default.nbits_calls == {"fused": 0, "torch": 1}
