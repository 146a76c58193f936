"""`GraphRunner(matmul_nbits="fused+float_zp")` / `"fused+float_zp+decode"` and `perplexity(..., matmul_nbits=...)`: a MatMulNBits
node with floating-point zero points (an HQQ file) and a block size that is a multiple of 32 runs from its blob at any number of
rows (`ops.matmul_nbits_float_zp`) and is counted under `nbits_calls["float_zp"]`; every other node goes where "fused" /
"fused+decode" send it.  Three files of one tiny language model, built here: HQQ uint4 g = 32, RTN uint4 g = 32, HQQ uint4 g = 16."""
import numpy as np
import pytest
import torch

import onnx_quantize_amd as oq
from onnx_quantize_amd import HqqConfig, QConfig, QuantType, QWeightArgs, quantize
from onnx_quantize_amd import onnx_proto as P
from onnx_quantize_amd.graph_runner import GraphRunner

pytestmark = pytest.mark.gpu

VOCAB, WIDTH, LENGTH = 64, 64, 50
MODES = ("fused+float_zp", "fused+float_zp+decode")


def tiny_lm():
    """Gather(emb [64, 64], input_ids) -> MatMul(W [64, 64]) -> logits, |logits| around 10 or less."""
    rng = np.random.default_rng(0)
    emb = rng.standard_normal((VOCAB, WIDTH)).astype(np.float32)
    w = (rng.standard_normal((WIDTH, VOCAB)) * 0.4).astype(np.float32)
    nodes = [P.make_node("Gather", ["emb", "input_ids"], ["h"], name="embed", axis=0),
             P.make_node("MatMul", ["h", "W"], ["logits"], name="lm_head")]
    g = P.Message("GraphProto", name="tiny_lm", node=nodes, initializer=[P.numpy_to_tensor("emb", emb), P.numpy_to_tensor("W", w)],
                  input=[P.make_value_info("input_ids", P.DataType.INT64, [1, "T"])],
                  output=[P.make_value_info("logits", P.DataType.FLOAT, [1, "T", VOCAB])])
    return P.Message("ModelProto", ir_version=10, graph=g, opset_import=[P.Message("OperatorSetIdProto", domain="", version=21)])


def nbits_node(model):
    return next(n for n in model.graph.node if n.op_type == "MatMulNBits")


@pytest.fixture(scope="module")
def files():
    def weights(group, **kw):
        return QConfig(weights=QWeightArgs(dtype=QuantType.QUInt4, group_size=group, strategy="group", **kw))
    out = {"hqq32": quantize(tiny_lm(), weights(32, algorithm=HqqConfig())), "rtn32": quantize(tiny_lm(), weights(32)),
           "hqq16": quantize(tiny_lm(), weights(16, algorithm=HqqConfig()))}
    for name, model in out.items():
        node = nbits_node(model)
        inits = {t.name: t for t in model.graph.initializer}
        attrs = {a.name: P.attribute_value(a) for a in node.attribute}
        assert attrs["block_size"] == (16 if name == "hqq16" else 32)
        assert (inits[node.input[3]].data_type == P.DataType.FLOAT) == name.startswith("hqq")      # float zero points: the HQQ files
    return out


@pytest.fixture(scope="module")
def tokens():
    return np.random.default_rng(1).integers(0, VOCAB, LENGTH)


def feed_of(tokens, n):
    return torch.from_numpy(tokens[:n].astype(np.int64)).reshape(1, -1)


def float64_bounds(model, a):
    """Y64 of the file's own initializers and the A the runner fed the node, the bound of DESIGN.md 4.30 (an fp32 A) and a bound of
    the expansion route: every weight is fl(fl(q - zp) * s), two roundings, and an fp32 dot product of K terms adds K in any order --
    (K + 2) 2^-24 S to first order, doubled: (K + 2) 2^-23 S, S = |a| |w|."""
    node = nbits_node(model)
    inits = {t.name: P.tensor_to_numpy(t) for t in model.graph.initializer}
    attrs = {a_.name: P.attribute_value(a_) for a_ in node.attribute}
    K, N, g = attrs["K"], attrs["N"], attrs["block_size"]
    blocks = K // g
    blob = inits[node.input[1]].reshape(N, blocks, g // 2)
    q = np.stack([blob & 0xF, blob >> 4], axis=-1).reshape(N, blocks, g).astype(np.float64)
    zraw = inits[node.input[3]]
    assert zraw.dtype == np.float32
    zp = zraw.reshape(N, blocks)
    zi = np.clip(np.rint(zp), 0, 15).astype(np.float32)                  # the kernel's split, in float32
    f = (zp - zi).astype(np.float64)
    scales = inits[node.input[2]].reshape(N, blocks, 1).astype(np.float64)
    a64 = a.reshape(-1, K).double().cpu().numpy()
    w64 = ((q - zp.astype(np.float64)[:, :, None]) * scales).reshape(N, K)
    y64 = a64 @ w64.T
    wm = ((np.abs(q - zi.astype(np.float64)[:, :, None]) + np.abs(f)[:, :, None]) * np.abs(scales)).reshape(N, K)
    s = np.abs(a64) @ wm.T
    term = (K + 3 * blocks + 4) * 2.0 ** -23 * s + 2.0 ** -21 * s + K * 2.0 ** -38 * np.abs(a64).max(axis=1, keepdims=True) * wm.max()
    expansion = (K + 2) * 2.0 ** -23 * (np.abs(a64) @ np.abs(w64).T)
    return y64, term + 2.0 ** -24 * (np.abs(y64) + term), expansion + 2.0 ** -24 * (np.abs(y64) + expansion)


@pytest.mark.parametrize("n_tokens", [17, 50])
def test_an_hqq_file_runs_from_its_blob_past_16_rows_and_the_logits_hold_the_bound(files, tokens, n_tokens):
    model = files["hqq32"]
    node = nbits_node(model)
    feed = feed_of(tokens, n_tokens)
    runner = GraphRunner(model, outputs=[node.input[0], "logits"], device="cuda", matmul_nbits="fused+float_zp")
    got = runner(feed)
    assert runner.nbits_calls == {"fused": 0, "torch": 0, "float_zp": 1}
    assert got["logits"].shape == (1, n_tokens, VOCAB)
    y64, bound, expansion_bound = float64_bounds(model, got[node.input[0]])
    logits = got["logits"].reshape(-1, VOCAB).double().cpu().numpy()
    err = np.abs(logits - y64)
    assert np.abs(y64).max() < 40 and (err <= bound).all(), (err - bound).max()
    default = GraphRunner(model, device="cuda")
    plain = default(feed)["logits"].reshape(-1, VOCAB).double().cpu().numpy()
    assert default.nbits_calls == {"fused": 0, "torch": 1}
    apart = np.abs(logits - plain)
    assert (apart <= bound + expansion_bound).all(), (apart - bound - expansion_bound).max()


@pytest.mark.parametrize("n_tokens", [1, 5, 16, 17])
def test_with_decode_the_first_16_rows_go_to_the_decode_kernel_and_17_to_the_float_zp_one(files, tokens, n_tokens):
    runner = GraphRunner(files["hqq32"], device="cuda", matmul_nbits="fused+float_zp+decode")
    got = runner(feed_of(tokens, n_tokens))["logits"]
    route = "decode" if n_tokens <= 16 else "float_zp"
    assert runner.nbits_calls == {"fused": 0, "torch": 0, "float_zp": 0, "decode": 0, route: 1}
    other = GraphRunner(files["hqq32"], device="cuda", matmul_nbits="fused+decode" if n_tokens <= 16 else "fused+float_zp")
    assert torch.equal(got.view(torch.uint8), other(feed_of(tokens, n_tokens))["logits"].view(torch.uint8))


@pytest.mark.parametrize("n_tokens", [5, 17])
@pytest.mark.parametrize("mode", MODES)
def test_an_rtn_file_gives_the_bytes_and_the_counts_of_the_mode_without_float_zp(files, tokens, mode, n_tokens):
    feed = feed_of(tokens, n_tokens)
    base = mode.replace("+float_zp", "")
    runner, plain = GraphRunner(files["rtn32"], device="cuda", matmul_nbits=mode), GraphRunner(files["rtn32"], device="cuda", matmul_nbits=base)
    a, b = runner(feed)["logits"], plain(feed)["logits"]
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert runner.nbits_calls == {**plain.nbits_calls, "float_zp": 0}
    assert sum(plain.nbits_calls.values()) == 1 and plain.nbits_calls["torch"] == 0


@pytest.mark.parametrize("mode", MODES)
def test_an_hqq_file_of_group_16_goes_to_the_expansion_route_past_16_rows(files, tokens, mode):
    feed = feed_of(tokens, 17)
    runner, default = GraphRunner(files["hqq16"], device="cuda", matmul_nbits=mode), GraphRunner(files["hqq16"], device="cuda")
    a, b = runner(feed)["logits"], default(feed)["logits"]
    assert runner.nbits_calls == {k: int(k == "torch") for k in runner.nbits_calls} and runner.nbits_calls["float_zp"] == 0
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_the_older_modes_keep_their_counters_and_their_routes(files, tokens):
    for mode, keys in (("torch", ["fused", "torch"]), ("fused", ["fused", "torch"]), ("fused+decode", ["decode", "fused", "torch"])):
        runner = GraphRunner(files["hqq32"], device="cuda", matmul_nbits=mode)
        runner(feed_of(tokens, 17))
        assert sorted(runner.nbits_calls) == keys and runner.nbits_calls["torch"] == 1


def test_a_float_zp_pass_is_recordable_and_replays_bit_for_bit(files, tokens):
    feed = feed_of(tokens, 50)
    eager = GraphRunner(files["hqq32"], device="cuda", matmul_nbits="fused+float_zp")
    rec = GraphRunner(files["hqq32"], device="cuda", matmul_nbits="fused+float_zp", capture=True)
    want = eager(feed)["logits"]
    for i in range(4):
        assert torch.equal(want, rec(feed)["logits"]), i
    assert next(iter(rec._graphs.values())) is not None, "a pass with the float-zp kernel synchronises with nothing: it can be recorded"


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


@pytest.mark.parametrize("mode", MODES)
def test_perplexity_passes_the_value_through(files, tokens, mode):
    runner = GraphRunner(files["hqq32"], device="cuda", matmul_nbits=mode)
    want = restated_perplexity(runner, tokens, 24, 12)                   # windows of 24 tokens and a last one of 14: every node past or at the decode rows
    assert runner.nbits_calls["float_zp"] >= 1 and runner.nbits_calls["fused"] == 0 and runner.nbits_calls["torch"] == 0
    got = oq.perplexity(files["hqq32"], tokens, max_length=24, stride=12, matmul_nbits=mode)
    assert abs(got - want) <= 1e-9 * want, (got, want)
    assert np.isfinite(got) and got > 1.0


def test_a_cpu_runner_degrades_and_unknown_values_are_refused(files):
    for mode in MODES:
        cpu = GraphRunner(files["hqq32"], device="cpu", matmul_nbits=mode)
        assert cpu.matmul_nbits == "torch" and cpu.nbits_calls == {"fused": 0, "torch": 0}
    for value in ("float_zp", "fused+decode+float_zp", "torch+float_zp"):
        with pytest.raises(ValueError, match="matmul_nbits"):
            GraphRunner(files["hqq32"], device="cuda", matmul_nbits=value)
