"""`GraphRunner(matmul_nbits="fused+decode")` and `perplexity(..., matmul_nbits="fused+decode")`: a MatMulNBits node whose flattened
A has at most 16 rows runs on the decode kernel (`ops.matmul_nbits_decode`) -- HQQ files (float zero points) and block size 16
included, which "fused" leaves on the expansion route -- and every other node goes as under "fused".  Three files of one tiny
language model: RTN uint4 g = 32, HQQ uint4 g = 32, RTN uint4 g = 16."""
import numpy as np
import pytest
import torch

import onnx_quantize_amd as oq
from onnx_quantize_amd import HqqConfig, QConfig, QuantType, QWeightArgs, quantize
from onnx_quantize_amd import onnx_proto as P
from onnx_quantize_amd.graph_runner import GraphRunner

pytestmark = pytest.mark.gpu

VOCAB, WIDTH, LENGTH = 64, 64, 50
FILES = ("rtn32", "hqq32", "rtn16")
ROUTE_PAST_16_ROWS = {"rtn32": "fused", "hqq32": "torch", "rtn16": "torch"}


def tiny_lm():
    rng = np.random.default_rng(0)
    emb = rng.standard_normal((VOCAB, WIDTH)).astype(np.float32)
    w = (rng.standard_normal((WIDTH, VOCAB)) * 0.4).astype(np.float32)
    nodes = [P.make_node("Gather", ["emb", "input_ids"], ["h"], name="embed", axis=0),
             P.make_node("MatMul", ["h", "W"], ["logits"], name="lm_head")]
    g = P.Message("GraphProto", name="tiny_lm", node=nodes, initializer=[P.numpy_to_tensor("emb", emb), P.numpy_to_tensor("W", w)],
                  input=[P.make_value_info("input_ids", P.DataType.INT64, [1, "T"])],
                  output=[P.make_value_info("logits", P.DataType.FLOAT, [1, "T", VOCAB])])
    return P.Message("ModelProto", ir_version=10, graph=g, opset_import=[P.Message("OperatorSetIdProto", domain="", version=21)])


@pytest.fixture(scope="module")
def files():
    def weights(group, **kw):
        return QConfig(weights=QWeightArgs(dtype=QuantType.QUInt4, group_size=group, strategy="group", **kw))
    out = {"rtn32": quantize(tiny_lm(), weights(32)), "hqq32": quantize(tiny_lm(), weights(32, algorithm=HqqConfig())),
           "rtn16": quantize(tiny_lm(), weights(16))}
    for name, model in out.items():
        node = nbits_node(model)
        inits = {t.name: t for t in model.graph.initializer}
        attrs = {a.name: P.attribute_value(a) for a in node.attribute}
        assert attrs["block_size"] == (16 if name == "rtn16" else 32)
        assert (inits[node.input[3]].data_type == P.DataType.FLOAT) == (name == "hqq32")      # float zero points: the HQQ file only
    return out


@pytest.fixture(scope="module")
def tokens():
    return np.random.default_rng(1).integers(0, VOCAB, LENGTH)


def nbits_node(model):
    return next(n for n in model.graph.node if n.op_type == "MatMulNBits")


def feed_of(tokens, n):
    return torch.from_numpy(tokens[:n].astype(np.int64)).reshape(1, -1)


def float64_bound(model, a):
    """Y64 and the bound of DESIGN.md 4.26 for the file's own initializers and the A the runner fed the node."""
    node = nbits_node(model)
    inits = {t.name: P.tensor_to_numpy(t) for t in model.graph.initializer}
    attrs = {a_.name: P.attribute_value(a_) for a_ in node.attribute}
    K, N, g = attrs["K"], attrs["N"], attrs["block_size"]
    blocks = K // g
    blob = inits[node.input[1]].reshape(N, blocks, g // 2)
    q = np.stack([blob & 0xF, blob >> 4], axis=-1).reshape(N, blocks, g).astype(np.float64)
    zraw = inits[node.input[3]]
    if zraw.dtype.kind == "f":
        zp = zraw.reshape(N, blocks).astype(np.float64)
    else:
        zb = zraw.reshape(N, -1)
        zp = np.stack([zb & 0xF, zb >> 4], axis=-1).reshape(N, -1)[:, :blocks].astype(np.float64)
    scales = inits[node.input[2]].reshape(N, blocks, 1).astype(np.float64)
    a64 = a.reshape(-1, K).double().cpu().numpy()
    y64 = a64 @ ((q - zp[:, :, None]) * scales).reshape(N, K).T
    if zraw.dtype.kind == "f":
        s = np.abs(a64) @ ((q + np.abs(zp)[:, :, None]) * np.abs(scales)).reshape(N, K).T
    else:
        s = np.abs(a64) @ np.abs((q - zp[:, :, None]) * scales).reshape(N, K).T
    term = (g + blocks + 8) * 2.0 ** -24 * s
    return y64, term + 2.0 ** -24 * (np.abs(y64) + term)


@pytest.mark.parametrize("n_tokens", [1, 16])
@pytest.mark.parametrize("name", FILES)
def test_up_to_16_tokens_every_node_runs_on_the_decode_kernel_and_the_logits_hold_its_bound(files, tokens, name, n_tokens):
    model = files[name]
    node = nbits_node(model)
    runner = GraphRunner(model, outputs=[node.input[0], "logits"], device="cuda", matmul_nbits="fused+decode")
    got = runner(feed_of(tokens, n_tokens))
    assert runner.nbits_calls == {"fused": 0, "torch": 0, "decode": 1}
    y64, bound = float64_bound(model, got[node.input[0]])
    err = np.abs(got["logits"].reshape(-1, VOCAB).double().cpu().numpy() - y64)
    assert got["logits"].shape == (1, n_tokens, VOCAB)
    assert np.abs(y64).max() < 40 and (err <= bound).all(), (err - bound).max()


@pytest.mark.parametrize("name", FILES)
def test_17_tokens_go_as_under_fused_byte_for_byte(files, tokens, name):
    model, feed = files[name], feed_of(tokens, 17)
    runner, fused = (GraphRunner(model, device="cuda", matmul_nbits=mode) for mode in ("fused+decode", "fused"))
    a, b = runner(feed)["logits"], fused(feed)["logits"]
    expected = {"fused": 0, "torch": 0, "decode": 0, ROUTE_PAST_16_ROWS[name]: 1}
    assert runner.nbits_calls == expected
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_the_other_modes_keep_their_two_counters(files, tokens):
    for mode in ("torch", "fused"):
        runner = GraphRunner(files["rtn32"], device="cuda", matmul_nbits=mode)
        runner(feed_of(tokens, 4))
        assert sorted(runner.nbits_calls) == ["fused", "torch"] and sum(runner.nbits_calls.values()) == 1
    assert sorted(GraphRunner(files["rtn32"], device="cuda").nbits_calls) == ["fused", "torch"]


@pytest.mark.parametrize("name", FILES)
def test_a_decode_pass_is_recordable_and_replays_bit_for_bit(files, tokens, name):
    feed = feed_of(tokens, 16)
    eager = GraphRunner(files[name], device="cuda", matmul_nbits="fused+decode")
    rec = GraphRunner(files[name], device="cuda", matmul_nbits="fused+decode", capture=True)
    want = eager(feed)["logits"]
    for i in range(4):
        assert torch.equal(want, rec(feed)["logits"]), i
    assert next(iter(rec._graphs.values())) is not None, "a pass with the decode kernel synchronises with nothing: it can be recorded"


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
    return float(np.exp(total / count))


@pytest.mark.parametrize("name", FILES)
def test_perplexity_passes_the_value_through(files, tokens, name):
    runner = GraphRunner(files[name], device="cuda", matmul_nbits="fused+decode")
    want = restated_perplexity(runner, tokens, 16, 8)
    assert runner.nbits_calls["decode"] >= 1 and runner.nbits_calls["fused"] == 0 and runner.nbits_calls["torch"] == 0
    got = oq.perplexity(files[name], tokens, max_length=16, stride=8, matmul_nbits="fused+decode")
    assert abs(got - want) <= 1e-9 * want, (got, want)
    assert np.isfinite(got) and got > 1.0


def test_a_cpu_runner_degrades_and_unknown_values_are_refused(files):
    cpu = GraphRunner(files["rtn32"], device="cpu", matmul_nbits="fused+decode")
    assert cpu.matmul_nbits == "torch" and cpu.nbits_calls == {"fused": 0, "torch": 0}
    with pytest.raises(ValueError, match="matmul_nbits"):
        GraphRunner(files["rtn32"], device="cuda", matmul_nbits="decode")
