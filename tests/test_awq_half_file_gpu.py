"""AWQ / SmoothQuant on FLOAT16 files: `quantize(fp16_file, ..., preprocessors=[...], half_weights="native_calibrated")`.

The calibration walk runs the FLOAT16 graph as it is and folds its fp16 activations into `ops.SearchStatistics`; the searches read
the fp16 weight as it is (the `_h16` entry points); the `Mul` initializer is FLOAT16, r16 = fp16(1 / s), and the weight is rescaled
in fp32 by s_eff = 1 / fp32(r16); the clip search and RTN run on that fp32 matrix; MatMulNBits keeps FLOAT16
scales.  Every file here is the COMPOSITION of the public `ops` functions, byte for byte.

Inputs: w = (randn(256, 64) * 0.05) as fp16; x = randn(128, 256) * uniform(0.1, 4, 256) with 8 random channels times 30, rounded
to fp16 (numpy default_rng(SEED)).  tests/test_awq_half_abi.py checks on the CPU what makes the seed a test: the oracle's best
candidate lies inside the grid, wins clearly, and every r16 is a normal fp16."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 3
K, N, G = 256, 64, 32


def case(seed=SEED, k=K, n=N):
    r = np.random.default_rng(seed)
    w = (r.standard_normal((k, n)) * 0.05).astype(np.float16)
    x = r.standard_normal((128, k)) * r.uniform(0.1, 4, k)
    x[:, r.choice(k, 8, replace=False)] *= 30
    return w, x.astype(np.float16)


def _weights(**kw):
    from onnx_quantize_amd import QuantType, QWeightArgs
    return QWeightArgs(dtype=QuantType.QUInt4, group_size=G, strategy="group", **kw)


def _qc(x, pre=None):
    """All 128 rows in one batch: the statistics see them in one `add`."""
    from onnx_quantize_amd import CalibrationParams, QConfig
    if pre is None:
        return QConfig(weights=_weights())
    return QConfig(weights=_weights(), preprocessors=[pre], calibration_data=x, calibration_params=CalibrationParams(num_samples=128, batch_size=128))


def _inits(model):
    from onnx_quantize_amd.onnx_proto import tensor_to_numpy
    return {t.name: tensor_to_numpy(t) for t in model.graph.initializer}, {t.name: t.data_type for t in model.graph.initializer}


def _run(model, x, device):
    """Y of a parsed model on the rows `x` (GraphRunner), as float64."""
    import torch
    from onnx_quantize_amd.graph_runner import GraphRunner
    out = model.graph.output[0].name
    got = GraphRunner(model, outputs=[out], device=device)({model.graph.input[0].name: torch.from_numpy(np.ascontiguousarray(x))})
    return got[out].double().cpu().numpy()


def _s_eff(s):
    r16 = (np.float32(1) / s.astype(np.float32)).astype(np.float16)
    return r16, np.float32(1) / r16.astype(np.float32)


def _expect_node(model, node, w_eff, ratio):
    """The blob, zero points and FLOAT16 scales of `node` are those of ops.rtn_quantize on the fp32 matrix `w_eff` (device)."""
    from onnx_quantize_amd.hip import ops
    from onnx_quantize_amd.onnx_proto import DataType
    vals, types = _inits(model)
    k, n = w_eff.shape
    q, s, z = ops.rtn_quantize(w_eff, "uint4", "group", G, clip_ratio=ratio)
    assert vals[node.input[1]].tobytes() == ops.pack_matmul_nbits(q, G, 4).cpu().numpy().tobytes(), node.name
    assert vals[node.input[3]].tobytes() == ops.pack_zero_points_u4(z.reshape(-1), n, k // G).cpu().numpy().tobytes(), node.name
    assert types[node.input[2]] == DataType.FLOAT16
    assert vals[node.input[2]].tobytes() == s.cpu().numpy().astype(np.float16).reshape(n, k // G).tobytes(), node.name


def _quantize_half(w_list, qc):
    from half_model_helpers import half_model
    from onnx_quantize_amd import quantize
    from onnx_quantize_amd.onnx_proto import parse_model, serialize
    return parse_model(quantize(serialize(half_model(w_list)), qc, half_weights="native_calibrated"))


def test_awq_with_clip_search_is_the_composition_and_beats_rtn():
    import oq_oracle as O
    import torch
    from half_model_helpers import half_model
    from onnx_model_helpers import q_oracle
    from onnx_quantize_amd import AwqConfig, quantize
    from onnx_quantize_amd.hip import ops
    from onnx_quantize_amd.onnx_proto import DataType, parse_model, serialize

    w, x = case()
    w32, x32 = w.astype(np.float32), x.astype(np.float32)

    # the quality condition on the fp32 twin with the oracle as provider, first: a failure below then says which side broke it
    twin = half_model([w32])
    y = _run(twin, x32, "cpu")
    e_twin_awq = np.linalg.norm(y - _run(q_oracle(half_model([w32]), _qc(x32, AwqConfig(clip_search=True))), x32, "cpu"))
    e_twin_rtn = np.linalg.norm(y - _run(q_oracle(half_model([w32]), _qc(x32)), x32, "cpu"))
    print(f"fp32 twin, oracle: ||Y - Y_awq|| {e_twin_awq:.4f}, ||Y - Y_rtn|| {e_twin_rtn:.4f}")
    assert e_twin_awq <= e_twin_rtn

    out = _quantize_half([w], _qc(x, AwqConfig(clip_search=True)))
    assert [n.op_type for n in out.graph.node] == ["Mul", "MatMulNBits"]
    mul, node = out.graph.node
    vals, types = _inits(out)

    # the composition of the public functions
    xd, wd = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    stats = ops.SearchStatistics(K, "cuda")
    stats.add(xd)
    s, losses = ops.awq_scale_search_stats(stats, wd, "uint4", "group", G)
    s = s.cpu().numpy()
    assert 0 < int(np.argmin(losses)) < 19
    r16, s_eff = _s_eff(s)
    assert types[mul.input[1]] == DataType.FLOAT16
    assert vals[mul.input[1]].tobytes() == r16.tobytes()
    assert np.abs(s_eff / s - 1).max() <= 2.0 ** -11
    w_eff = torch.from_numpy(s_eff).cuda().reshape(-1, 1) * wd.float()
    stats.divide(torch.from_numpy(s_eff))
    ratio, _ = ops.awq_clip_search_stats(stats, w_eff, "uint4", "group", G)
    _expect_node(out, node, w_eff, ratio)

    # the quality condition on the files, on the calibration rows
    src = serialize(half_model([w]))
    rtn = parse_model(quantize(src, _qc(x), half_weights="native"))
    y16 = _run(half_model([w]), x, "cuda")
    e_awq, e_rtn = np.linalg.norm(y16 - _run(out, x, "cuda")), np.linalg.norm(y16 - _run(rtn, x, "cuda"))
    print(f"FLOAT16 files: ||Y - Y_awq|| {e_awq:.4f}, ||Y - Y_rtn|| {e_rtn:.4f}")
    assert e_awq <= e_rtn
    # and the oracle agrees with the search on the upcast inputs about the scale, to the bar of tests/test_preprocessing.py
    es, el = O.awq_scale_search(x32, w32, "uint4", "group", G)
    if int(np.argmin(el)) == int(np.argmin(losses)):
        np.testing.assert_allclose(s, es, rtol=2e-5)


def test_awq_without_clip_search_and_smooth_quant_are_the_composition():
    import torch
    from onnx_quantize_amd import AwqConfig, SmoothQuantConfig
    from onnx_quantize_amd.hip import ops
    from onnx_quantize_amd.onnx_proto import DataType

    w, x = case()
    xd, wd = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    stats = ops.SearchStatistics(K, "cuda")
    stats.add(xd)
    for pre, s in ((AwqConfig(clip_search=False), ops.awq_scale_search_stats(stats, wd, "uint4", "group", G)[0]),
                   (SmoothQuantConfig(alpha=0.5), ops.smooth_quant_scale_stats(stats, wd, 0.5))):
        out = _quantize_half([w], _qc(x, pre))
        assert [n.op_type for n in out.graph.node] == ["Mul", "MatMulNBits"]
        mul, node = out.graph.node
        vals, types = _inits(out)
        r16, s_eff = _s_eff(s.cpu().numpy())
        assert types[mul.input[1]] == DataType.FLOAT16
        assert vals[mul.input[1]].tobytes() == r16.tobytes()
        _expect_node(out, node, torch.from_numpy(s_eff).cuda().reshape(-1, 1) * wd.float(), 1.0)


def test_a_chain_taps_the_fp16_activation_in_mid_graph():
    """X -> MatMul(W0) -> H0 -> MatMul(W1): the second node's statistics are those of the fp16 value H0 the walk produced."""
    import torch
    from half_model_helpers import half_model
    from onnx_quantize_amd import AwqConfig
    from onnx_quantize_amd.graph_runner import GraphRunner
    from onnx_quantize_amd.hip import ops
    from onnx_quantize_amd.onnx_proto import DataType

    w0, x = case()
    w1 = (np.random.default_rng(SEED + 100).standard_normal((N, 96)) * 0.05).astype(np.float16)
    out = _quantize_half([w0, w1], _qc(x, AwqConfig(clip_search=False)))
    assert [n.op_type for n in out.graph.node] == ["Mul", "MatMulNBits", "Mul", "MatMulNBits"]
    vals, types = _inits(out)

    xd = torch.from_numpy(x).cuda()
    h0 = GraphRunner(half_model([w0, w1]), outputs=["H0"], device="cuda", capture=True, matmul="pieces")({"X": xd})["H0"]
    assert h0.dtype == torch.float16 and tuple(h0.shape) == (128, N)
    for i, (wi, xi) in enumerate(((w0, xd), (w1, h0))):
        wd = torch.from_numpy(wi).cuda()
        stats = ops.SearchStatistics(wi.shape[0], "cuda")
        stats.add(xi)
        s = ops.awq_scale_search_stats(stats, wd, "uint4", "group", G)[0].cpu().numpy()
        r16, s_eff = _s_eff(s)
        mul, node = out.graph.node[2 * i], out.graph.node[2 * i + 1]
        assert types[mul.input[1]] == DataType.FLOAT16
        assert vals[mul.input[1]].tobytes() == r16.tobytes(), i
        _expect_node(out, node, torch.from_numpy(s_eff).cuda().reshape(-1, 1) * wd.float(), 1.0)


def test_a_reciprocal_that_overflows_fp16_is_refused_by_node_and_channel():
    """One activation channel scaled down until its SmoothQuant scale is below 1 / 65504: fp16(1 / s) is infinite."""
    from onnx_quantize_amd import SmoothQuantConfig

    w, x = case()
    x = x.copy()
    x[:, 5] = np.float16(2.0 ** -24) * np.sign(x[:, 5].astype(np.float32)).astype(np.float16)     # max |x| = 6e-8 (a subnormal fp16)
    with pytest.raises(ValueError, match=r"node 'fc0'.*channel 5"):
        _quantize_half([w], _qc(x, SmoothQuantConfig(alpha=1.0)))
