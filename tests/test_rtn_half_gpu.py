"""RTN on fp16 / bf16 weights read as they are (csrc/rtn_half.hip, oq_rtn_quantize_h16).

Both conversions to fp32 are exact, so the yardstick is the unchanged oracle on ``W.astype(np.float32)`` (bf16 is upcast here
by shifting its bit patterns): integers and zero points equal, scales equal as bytes; and the fp32 kernels of this package on
``w.float()``, bit for bit, wherever a case has such a route.

The shapes are the smallest at which the kernels can go wrong: one group in a sliver of a column tile, a full and a ragged
column tile (the wave kernel's tile is 64 columns, a block's 256), every group size with a build of its own, the tallest fused
group, odd N with an odd leading dimension (2-byte loads), strided rows, and the channel / tensor / tall-group route."""
import types

import numpy as np
import pytest

import oq_oracle as O

pytestmark = pytest.mark.gpu

WTYPES = ["float16", "bfloat16"]


@pytest.fixture(scope="module")
def ops():
    import torch
    from onnx_quantize_amd.hip import ops as _ops
    assert torch.cuda.is_available()
    return _ops


# ------------------------------------------------------------------------------------ 2-byte matrices as uint16 bit patterns
def to_bits(w32, wtype):
    """fp32 -> the 2-byte type's bit patterns (fp16: round to nearest; bf16: truncation -- any 2-byte value will do)."""
    if wtype == "float16":
        with np.errstate(over="ignore"):
            return np.ascontiguousarray(w32, np.float32).astype(np.float16).view(np.uint16)
    return (np.ascontiguousarray(w32, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def upcast(bits, wtype):
    if wtype == "float16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def dev(bits, wtype):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda()
    return t.view(torch.float16 if wtype == "float16" else torch.bfloat16)


def make_bits(wtype, k, n, g, seed, nan_at=None):
    """Values placed per group (column n, k-group kg: case (n * kgroups + kg) % 5), so the groups of one matrix differ:
    uniform random | all zero | all equal | the type's largest magnitudes next to subnormals and -0.0 | integers and
    half-integers (x / s lands on exact ties)."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1.0, 1.0, size=(k, n)).astype(np.float32)
    bits = to_bits(w, wtype)
    big = 0x7BFF if wtype == "float16" else 0x7F7F           # 65504 | 3.39e38
    kgroups = k // g
    for col in range(n):
        for kg in range(kgroups):
            case = (col * kgroups + kg) % 5
            rows = slice(kg * g, kg * g + g)
            if case == 1:
                bits[rows, col] = 0
            elif case == 2:
                bits[rows, col] = to_bits(np.float32([0.37]), wtype)[0]
            elif case == 3:
                pat = np.array([big, big | 0x8000, 0x0001, 0x8001, 0x8000, 0x0000, 0x03FF if wtype == "float16" else 0x007F], np.uint16)
                bits[rows, col] = pat[np.arange(g) % len(pat)]
            elif case == 4:
                vals = (rng.integers(-30, 31, size=g) * 0.5).astype(np.float32)
                bits[rows, col] = to_bits(vals, wtype)
    if nan_at is not None:
        bits[nan_at] = 0x7E00 if wtype == "float16" else 0x7FC0
    return bits


def oracle(w32, qtype, strategy, g, sym, rr, clip):
    with np.errstate(all="ignore"):
        return O.rtn_quantize(w32, qtype, strategy, g, sym, rr, clip)


def check_against_oracle_and_fp32(ops, bits, wtype, qtype, strategy, g, sym=False, rr=False, clip=1.0, layout="kn", view=None):
    """``view``: a function applied to the device tensor and the host array alike (strided / offset views)."""
    import torch
    wd = dev(bits, wtype)
    w32 = upcast(bits, wtype)
    if view is not None:
        wd, w32 = view(wd), view(w32)
    q, s, z = ops.rtn_quantize(wd, qtype, strategy, g, sym, rr, clip, False, layout=layout)
    fq, fs, fz = ops.rtn_quantize(wd.float(), qtype, strategy, g, sym, rr, clip, False, layout=layout)
    assert q.dtype == fq.dtype and q.shape == fq.shape and s.shape == fs.shape and z.shape == fz.shape and z.dtype == fz.dtype
    assert s.dtype == torch.float32
    assert torch.equal(q, fq), "integers differ from the fp32 kernels on w.float()"
    assert torch.equal(z, fz)
    assert s.cpu().numpy().tobytes() == fs.cpu().numpy().tobytes()
    eq, es, ez = oracle(np.ascontiguousarray(w32), qtype, strategy, g, sym, rr, clip)
    assert s.cpu().numpy().tobytes() == np.asarray(es, np.float32).tobytes(), "scales differ from the oracle"
    np.testing.assert_array_equal(z.cpu().numpy(), ez)
    if layout == "kn":
        np.testing.assert_array_equal(q.cpu().numpy(), eq)
    elif qtype in ("uint4", "uint8"):          # the oracle's blob is defined for the unsigned types MatMulNBits takes
        k = w32.shape[0]
        gg = k if g == -1 else min(g, k)
        blob, _, _ = O.matmul_nbits_layout(np.asarray(eq).astype(np.uint8), np.asarray(es), np.asarray(ez), gg, 4 if qtype == "uint4" else 8)
        np.testing.assert_array_equal(q.cpu().numpy(), blob)


GROUP_SHAPES = [(128, 8, 128), (256, 520, 128), (384, 1032, 16), (384, 1032, 32), (384, 1032, 64), (384, 1032, 128), (512, 16, 256)]


@pytest.mark.parametrize("wtype", WTYPES)
@pytest.mark.parametrize("layout", ["kn", "nbits"])
@pytest.mark.parametrize("shape", GROUP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_group_shapes(ops, wtype, layout, shape):
    k, n, g = shape
    bits = make_bits(wtype, k, n, g, seed=k + n + g)
    check_against_oracle_and_fp32(ops, bits, wtype, "uint4", "group", g, layout=layout)
    check_against_oracle_and_fp32(ops, bits, wtype, "int8", "group", g, sym=True, layout=layout)


@pytest.mark.parametrize("wtype", WTYPES)
@pytest.mark.parametrize("layout", ["kn", "nbits"])
@pytest.mark.parametrize("shape", GROUP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_group_shapes_row_strided(ops, wtype, layout, shape):
    """ldw > N: the matrix is a column range of a wider one (16-byte aligned rows, and rows off by one element)."""
    k, n, g = shape
    wide = make_bits(wtype, k, n + 24, g, seed=7 * k + n + g)
    check_against_oracle_and_fp32(ops, wide, wtype, "uint4", "group", g, layout=layout, view=lambda a: a[:, 8:8 + n])
    check_against_oracle_and_fp32(ops, wide, wtype, "uint8", "group", g, layout=layout, view=lambda a: a[:, 3:3 + n])


@pytest.mark.parametrize("wtype", WTYPES)
def test_odd_columns_and_odd_leading_dimension(ops, wtype):
    """N = 7 inside rows of 9 elements: no row is 16-byte aligned; the same kernel, 2-byte loads, the same bytes."""
    wide = make_bits(wtype, 128, 9, 128, seed=5)
    for qtype, sym in (("uint4", False), ("int4", True), ("uint8", False), ("int8", True)):
        check_against_oracle_and_fp32(ops, wide, wtype, qtype, "group", 128, sym=sym, view=lambda a: a[:, 1:8])


@pytest.mark.parametrize("wtype", WTYPES)
@pytest.mark.parametrize("qtype", ["uint4", "int4", "uint8", "int8"])
def test_types_and_flags(ops, wtype, qtype):
    bits = make_bits(wtype, 256, 72, 64, seed=11)
    for sym in (False, True):
        for rr in (False, True):
            for clip in (1.0, 0.8):
                for layout in ("kn", "nbits"):
                    check_against_oracle_and_fp32(ops, bits, wtype, qtype, "group", 64, sym, rr, clip, layout=layout)


@pytest.mark.parametrize("wtype", WTYPES)
def test_group_sizes_without_a_wave_build(ops, wtype):
    """g = 48 / 24 (K % g == 0, not a power of two): the thread-per-column fused kernel; g = 48 also as a blob."""
    bits = make_bits(wtype, 96, 70, 48, seed=3)
    check_against_oracle_and_fp32(ops, bits, wtype, "uint4", "group", 48)
    check_against_oracle_and_fp32(ops, bits, wtype, "uint4", "group", 48, layout="nbits")
    check_against_oracle_and_fp32(ops, bits, wtype, "int8", "group", 24, sym=True)


@pytest.mark.parametrize("wtype", WTYPES)
@pytest.mark.parametrize("strategy", ["channel", "tensor"])
@pytest.mark.parametrize("shape", [(200, 72), (1, 5)], ids=["200x72", "1x5"])
def test_channel_and_tensor(ops, wtype, strategy, shape):
    k, n = shape
    bits = make_bits(wtype, k, n, k, seed=k + n)
    for qtype, sym, rr, clip in (("uint4", False, False, 1.0), ("int8", True, False, 0.8), ("uint8", False, True, 1.0), ("int4", True, True, 1.0)):
        check_against_oracle_and_fp32(ops, bits, wtype, qtype, strategy, -1, sym, rr, clip)


@pytest.mark.parametrize("wtype", WTYPES)
def test_groups_taller_than_the_fused_kernels(ops, wtype):
    """g = 384 > 256: the range pass and the quantize pass; [K,N] bytes and (g % 128 == 0, N % 4 == 0) the blob."""
    bits = make_bits(wtype, 768, 72, 384, seed=9)
    check_against_oracle_and_fp32(ops, bits, wtype, "uint4", "group", 384)
    check_against_oracle_and_fp32(ops, bits, wtype, "uint4", "group", 384, layout="nbits")
    check_against_oracle_and_fp32(ops, bits, wtype, "uint4", "group", -1, layout="nbits")


@pytest.mark.parametrize("wtype", WTYPES)
def test_parameters_only(ops, wtype):
    bits = make_bits(wtype, 256, 72, 128, seed=2)
    for strategy, g in (("group", 128), ("channel", -1), ("tensor", -1)):
        q, s, z = ops.rtn_quantize(dev(bits, wtype), "uint4", strategy, g, emit_q=False)
        _, es, ez = oracle(upcast(bits, wtype), "uint4", strategy, g, False, False, 1.0)
        assert q is None and s.cpu().numpy().tobytes() == np.asarray(es, np.float32).tobytes()
        np.testing.assert_array_equal(z.cpu().numpy(), ez)


@pytest.mark.parametrize("wtype", WTYPES)
@pytest.mark.parametrize("shape", [(256, 72, 128, "group"), (256, 72, 32, "group"), (200, 72, -1, "channel")], ids=["g128", "g32", "channel"])
def test_a_nan_poisons_exactly_its_group(ops, wtype, shape):
    import torch
    k, n, g, strategy = shape
    clean = make_bits(wtype, k, n, k if g == -1 else g, seed=21)
    dirty = make_bits(wtype, k, n, k if g == -1 else g, seed=21, nan_at=(k // 2 + 3, 17))
    for layout in ("kn", "nbits") if strategy == "group" else ("kn",):
        q0, s0, z0 = ops.rtn_quantize(dev(clean, wtype), "uint4", strategy, g, layout=layout)
        q1, s1, z1 = ops.rtn_quantize(dev(dirty, wtype), "uint4", strategy, g, layout=layout)
        fq, fs, fz = ops.rtn_quantize(dev(dirty, wtype).float(), "uint4", strategy, g, layout=layout)
        s0, s1 = s0.cpu().numpy().reshape(-1), s1.cpu().numpy().reshape(-1)
        kgroups = 1 if g == -1 else k // g
        hit = 17 * kgroups + (0 if g == -1 else (k // 2 + 3) // g)
        assert np.isnan(s1[hit]) and not np.isnan(s0[hit])
        keep = np.arange(s1.size) != hit
        assert s1[keep].tobytes() == s0[keep].tobytes(), "a neighbouring group's scale changed"
        assert np.array_equal(np.isnan(s1), np.isnan(fs.cpu().numpy().reshape(-1)))
        assert torch.equal(z1.reshape(-1)[torch.from_numpy(keep).cuda()], z0.reshape(-1)[torch.from_numpy(keep).cuda()])
        assert torch.equal(q1, fq) and torch.equal(z1, fz)
        if layout == "kn":      # every column but the poisoned one, and the poisoned column's other groups
            same = torch.ones((k, n), dtype=torch.bool)
            rows = slice(0, k) if g == -1 else slice((k // 2 + 3) // g * g, (k // 2 + 3) // g * g + g)
            same[rows, 17] = False
            assert torch.equal(q1.cpu()[same], q0.cpu()[same])


# ------------------------------------------------------------------------------------ documented routes
@pytest.mark.parametrize("wtype", WTYPES)
def test_packed_nibbles_are_the_kn_route_and_the_packer(ops, wtype):
    import torch
    bits = make_bits(wtype, 256, 72, 128, seed=4)
    for qtype in ("uint4", "int4"):
        q, s, z = ops.rtn_quantize(dev(bits, wtype), qtype, "group", 128, layout="kn")
        p, ps, pz = ops.rtn_quantize(dev(bits, wtype), qtype, "group", 128, layout="kn_packed4")
        assert p.shape == (256, 36) and p.dtype == torch.uint8
        assert torch.equal(p.reshape(-1), ops.pack_nibbles(q)) and torch.equal(s, ps) and torch.equal(z, pz)
        fp, _, _ = ops.rtn_quantize(dev(bits, wtype).float(), qtype, "group", 128, layout="kn_packed4")
        assert torch.equal(p, fp)


@pytest.mark.parametrize("wtype", WTYPES)
def test_mse_and_straddling_groups_take_the_device_cast(ops, wtype):
    import torch
    bits = make_bits(wtype, 128, 40, 64, seed=6)
    got = ops.rtn_quantize(dev(bits, wtype), "uint4", "group", 64, mse=True)
    ref = ops.rtn_quantize(dev(bits, wtype).float(), "uint4", "group", 64, mse=True)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    bits = to_bits(np.random.default_rng(8).standard_normal((96, 4)).astype(np.float32), wtype)      # K % g != 0, K * N % g == 0
    got = ops.rtn_quantize(dev(bits, wtype), "uint4", "group", 64)
    ref = ops.rtn_quantize(dev(bits, wtype).float(), "uint4", "group", 64)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    eq, es, ez = oracle(upcast(bits, wtype), "uint4", "group", 64, False, False, 1.0)
    np.testing.assert_array_equal(got[0].cpu().numpy(), eq)
    assert got[1].cpu().numpy().tobytes() == es.tobytes()


def test_fp32_only_entry_points_say_so_by_name(ops):
    import torch
    w = torch.zeros((64, 16), dtype=torch.float16, device="cuda")
    with pytest.raises(TypeError, match="rtn_quantize_many"):
        ops.rtn_quantize_many([w], "uint4", 32)
    with pytest.raises(TypeError, match="rtn_quantize_batched"):
        ops.rtn_quantize_batched(w.reshape(1, 64, 16), "uint4", 32)
    with pytest.raises(TypeError, match="rtn_quantize_tensor_many"):
        ops.rtn_quantize_tensor_many([w], "uint4")


def test_library_refuses_what_it_has_no_kernel_for(ops):
    import torch
    from onnx_quantize_amd.hip import _lib as L
    lib = L.load()
    w = torch.zeros((96, 4), dtype=torch.float16, device="cuda")
    q = torch.empty((96, 4), dtype=torch.uint8, device="cuda")
    s = torch.empty(8, dtype=torch.float32, device="cuda")
    z = torch.empty(8, dtype=torch.uint8, device="cuda")
    args = lambda g, layout: (w.data_ptr(), L.OQ_W_F16, 96, 4, 4, L.OQ_UINT4, L.OQ_GROUP, g, 0, 0, 1.0, q.data_ptr(), s.data_ptr(),
                              z.data_ptr(), layout, None, 0, None)
    assert lib.oq_rtn_quantize_h16(*args(64, L.OQ_LAYOUT_KN)) == L.OQ_ERR_UNSUPPORTED and b"straddle" in lib.oq_last_error()
    assert lib.oq_rtn_quantize_h16(*args(32, L.OQ_LAYOUT_KN_PACKED4)) == L.OQ_ERR_UNSUPPORTED and b"oq_pack_nibbles" in lib.oq_last_error()


# ------------------------------------------------------------------------------------ the seam
class _Tensor:
    def __init__(self, a):
        self._a = np.asarray(a)

    def numpy(self):
        return self._a


class _Value:
    def __init__(self, name, const_value=None):
        self.name, self.const_value = name, const_value


@pytest.mark.parametrize("algorithm", ["rtn", "gptq", "hqq"])
@pytest.mark.parametrize("flagged", [False, True], ids=["plain", "matmul_nbits"])
def test_seam_takes_a_float16_weight(algorithm, flagged):
    """The three arrays for an np.float16 const_value are byte-identical to those for its fp32 copy; the same for resident
    fp16 / bf16 device values."""
    import torch
    from onnx_quantize_amd import GPTQConfig, HqqConfig, QConfig, QuantType, QWeightArgs, seam

    rng = np.random.default_rng(31)
    w16 = rng.standard_normal((256, 64)).astype(np.float16)
    x = rng.standard_normal((6, 10, 256)).astype(np.float32)           # the calibration input size of tests/test_seam.py
    kw = {"dtype": QuantType.from_string("uint4"), "group_size": 32}
    if algorithm == "gptq":
        kw["algorithm"] = GPTQConfig(block_size=32)
    elif algorithm == "hqq":
        kw.update(strategy="group", algorithm=HqqConfig(iters=10))
    qc = QConfig(weights=QWeightArgs(**kw))

    def run(value):
        node = types.SimpleNamespace(meta={"input": x})
        out = types.SimpleNamespace(producer=lambda node=node: node)
        return seam.weight_arrays(value, qc, out, flagged)

    seam.clear_shared_inputs()
    ref = run(_Value("fc.weight", _Tensor(w16.astype(np.float32))))
    got = run(_Value("fc.weight", _Tensor(w16)))
    assert got[1].dtype == np.dtype(qc.weights.scale_dtype) == np.float32
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    for dt in (torch.float16, torch.bfloat16):
        resident = torch.from_numpy(w16).cuda().to(dt)
        value = _Value("fc.weight", _Tensor(np.zeros((256, 64), np.float16)))
        value.device_value, value.placeholder = resident, True
        got = run(value)
        ref = run(_Value("fc.weight", _Tensor(resident.float().cpu().numpy())))
        for a, b in zip(got, ref):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    seam.clear_shared_inputs()


# ------------------------------------------------------------------------------------ the file path, opt-in
def _matmul_chain(w_list):
    from half_model_helpers import half_model
    return half_model(w_list)


def _dequantized(model, node):
    """(q - zp) * scale of one MatMulNBits node from its initializers, fp32 [K, N] on the host (uint4)."""
    from onnx_quantize_amd.onnx_proto import tensor_to_numpy
    inits = {t.name: t for t in model.graph.initializer}
    attrs = {a.name: a.i for a in node.attribute}
    K, N, g = attrs["K"], attrs["N"], attrs["block_size"]
    blocks = K // g
    blob = tensor_to_numpy(inits[node.input[1]]).reshape(N, blocks, g // 2)
    q = np.stack([blob & 0x0F, blob >> 4], axis=-1).reshape(N, blocks, g).astype(np.float32)
    s = tensor_to_numpy(inits[node.input[2]]).reshape(N, blocks).astype(np.float32)
    zb = tensor_to_numpy(inits[node.input[3]]).reshape(N, -1)
    z = np.stack([zb & 0x0F, zb >> 4], axis=-1).reshape(N, -1)[:, :blocks].astype(np.float32)
    return q, z, s, ((q - z[:, :, None]) * s[:, :, None]).reshape(N, K).T


def test_native_file_path_on_the_device_and_the_runner_on_fp16():
    import torch
    from onnx_quantize_amd import QConfig, QuantType, QWeightArgs, quantize
    from onnx_quantize_amd.graph_runner import GraphRunner
    from onnx_quantize_amd.model_quantize import quantize_model
    from onnx_quantize_amd.onnx_proto import parse_model, serialize
    from half_model_helpers import upcasting_oracle

    rng = np.random.default_rng(17)
    ws = [(rng.standard_normal((64, 128)) * 0.2).astype(np.float16), (rng.standard_normal((128, 64)) * 0.2).astype(np.float16)]
    src = serialize(_matmul_chain(ws))
    qc = lambda: QConfig(weights=QWeightArgs(dtype=QuantType.QUInt4, group_size=32, strategy="group"))      # noqa: E731
    got = quantize(src, qc(), half_weights="native")
    ref = serialize(quantize_model(src, qc(), weight_arrays=upcasting_oracle, quantize_bias=O.quantize_bias, half_weights="native"))
    assert got == ref, "the device file differs from the oracle-provider file"
    model = parse_model(got)
    assert [n.op_type for n in model.graph.node] == ["MatMulNBits", "MatMulNBits"]

    x = torch.from_numpy((rng.standard_normal((4, 64))).astype(np.float16)).cuda()
    y = GraphRunner(model, device="cuda")({"X": x})["Y"]
    assert y.dtype == torch.float16 and tuple(y.shape) == (4, 64)
    w0, w1 = (_dequantized(model, n)[3] for n in model.graph.node)
    # yardstick: torch's own fp16 matmul on the same dequantized matrices against the float64 product; the runner's only licence
    # is the rounding that product already has, with a margin of x 2
    t0, t1 = torch.from_numpy(w0).cuda().half(), torch.from_numpy(w1).cuda().half()
    torch_out = ((x @ t0) @ t1).double().cpu().numpy()
    exact = (x.double().cpu().numpy() @ t0.double().cpu().numpy()) @ t1.double().cpu().numpy()
    torch_err = np.abs(torch_out - exact).max()
    runner_err = np.abs(y.double().cpu().numpy() - exact).max()
    print(f"fp16 runner: max error {runner_err:.3e}, torch's fp16 product {torch_err:.3e}")
    assert torch_err > 0 and runner_err <= 2 * torch_err


def test_runner_matmul_nbits_on_fp32_is_the_written_out_product():
    """Regression guard of the runner's fp16 support: an fp32 A computes exactly what it computed before."""
    import torch
    from onnx_quantize_amd import QConfig, QuantType, QWeightArgs, quantize
    from onnx_quantize_amd.graph_runner import GraphRunner
    from onnx_quantize_amd.onnx_proto import parse_model, serialize

    rng = np.random.default_rng(18)
    w = rng.standard_normal((64, 24)).astype(np.float32)
    model = parse_model(quantize(serialize(_matmul_chain([w])), QConfig(weights=QWeightArgs(dtype=QuantType.QUInt4, group_size=32, strategy="group"))))
    node = model.graph.node[0]
    assert node.op_type == "MatMulNBits"
    x = torch.from_numpy(rng.standard_normal((5, 64)).astype(np.float32)).cuda()
    y = GraphRunner(model, device="cuda")({"X": x})["Y"]
    q, z, s, _ = _dequantized(model, node)
    qd, zd, sd = (torch.from_numpy(a).cuda() for a in (q, z, s))
    wd = ((qd - zd[:, :, None]) * sd[:, :, None]).reshape(24, 64)
    assert y.dtype == torch.float32 and torch.equal(y, x @ wd.t())
