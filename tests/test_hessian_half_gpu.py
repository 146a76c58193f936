"""The GPTQ Hessian straight from fp16 / bf16 activations (csrc/syrk_bf16x3.hip section 4, oq_hessian_accumulate_h16) and what
is built on it: `ops.hessian_accumulate` on half tensors, the calibration driver, `half_weights="native_calibrated"`.

Half x half products are exact in fp32, so integer data must come out bit for bit whatever the summation order, and random
data within the project's Hessian gate of float64 (1e-5 max |H|, tests/test_gptq_gpu.py).  The shapes are the smallest at
which the route can go wrong: K = 1, an odd leading dimension (2-byte loads), a strided view, ragged tiles in both extents,
and the row count at which T is first cut into slices."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ["float16", "bfloat16"]
# oq_hessian_accumulate_h16 cuts T into slices from two slices of >= 512 rows after padding to 32-row stages: 32 stages, i.e.
# 993 rows (31 * 32 + 1).  With K = 520 (six tiles against 256 CUs) the second slice is taken.
FIRST_SPLIT_ROWS = 993


@pytest.fixture(scope="module")
def ops():
    import torch
    from onnx_quantize_amd.hip import ops as _ops
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture
def restore_hessian_method(ops):
    before = ops.hessian_method()
    yield
    ops.hessian_set_method(before)


def tdtype(name):
    import torch
    return getattr(torch, name)


def half_of(x32, name):
    """fp32 NumPy -> (device tensor of the half type, its exact values as float64 NumPy)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x32, np.float32)).cuda().to(tdtype(name))
    return t, t.double().cpu().numpy()


# ------------------------------------------------------------------------------------ 1. exact integers
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(4, 512, 520), (4, 10, 9), (1, FIRST_SPLIT_ROWS, 520)], ids=["2048x520", "40x9", "first_split"])
def test_integer_data_is_exact_whatever_the_summation_order(ops, dtype, shape):
    """Integers in [-8, 8]: every partial sum stays below 2^24 and 2 / n is a power of two, so H equals the int64 result bit for
    bit.  Catches every indexing and padding error."""
    import torch
    n, _, k = shape
    xi = np.random.default_rng(sum(shape)).integers(-8, 9, size=shape)
    x = torch.from_numpy(xi.astype(np.float32)).cuda().to(tdtype(dtype))
    h = torch.full((k, k), 7.0, device="cuda")                      # beta = 0 on the first call: what H held is not read
    assert ops.hessian_accumulate(x, h, 0) == n
    x2 = xi.reshape(-1, k).astype(np.int64)
    assert x2.shape[0] * 64 < 2 ** 24 and n in (1, 2, 4)
    want = (x2.T @ x2).astype(np.float64) * (2.0 / n)
    np.testing.assert_array_equal(h.cpu().numpy().astype(np.float64), want)


# ------------------------------------------------------------------------------------ 2. random data against float64
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("t,k,ld", [(16, 1, 1), (64, 130, 131), (333, 200, 256), (2050, 1301, 1301), (4096, 1024, 1024)])
def test_random_data_against_float64(ops, dtype, t, k, ld):
    import torch
    rng = np.random.default_rng(t + k)
    x = rng.standard_normal((t, ld), dtype=np.float32) * rng.uniform(0.1, 3, size=ld).astype(np.float32) + 0.25
    if k > 8:
        x[:, 5] = 0
    # an odd leading dimension on an odd element offset: rows that are only 2-byte aligned
    flat = torch.zeros(t * ld + 1, dtype=tdtype(dtype), device="cuda")
    off = 1 if ld % 2 else 0
    flat[off:off + t * ld] = torch.from_numpy(x).cuda().to(tdtype(dtype)).reshape(-1)
    xd = flat[off:off + t * ld].reshape(t, ld)[:, :k]                # a strided view when ld > k
    if ld % 2 and ld > 1:
        assert xd.data_ptr() % 4 == 2 and xd.stride(0) % 2 == 1
    arg = xd.reshape(2, t // 2, k) if ld == k else xd
    n_add = 2 if ld == k else t
    h = torch.zeros((k, k), dtype=torch.float32, device="cuda")
    assert ops.hessian_accumulate(arg, h, 0) == n_add
    x64 = xd.double().cpu().numpy()
    ref = (2.0 / n_add) * x64.T @ x64
    bound = 1e-5 * float(np.abs(ref).max())
    got = h.cpu().numpy()
    print(f"{dtype} {t}x{k} ld {ld}: max |H - H64| = {np.abs(got - ref).max() / np.abs(ref).max():.3e} of max |H64|")
    np.testing.assert_allclose(got, ref, rtol=0, atol=bound)
    np.testing.assert_array_equal(got, got.T)
    if k > 8:
        assert np.all(got[5] == 0) and np.all(got[:, 5] == 0)
    assert ops.hessian_accumulate(arg, h, n_add) == 2 * n_add      # the running mean of the same X twice: the same H
    np.testing.assert_allclose(h.cpu().numpy(), ref, rtol=0, atol=bound)
    np.testing.assert_array_equal(h.cpu().numpy(), h.cpu().numpy().T)


# ------------------------------------------------------------------------------------ 3. dead channels
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_same_dead_channels_as_the_fp32_route(ops, restore_hessian_method, dtype):
    """gptq.py:284-286 calls a channel dead when H[k][k] == 0 (the expectations of
    test_hessian_f16_pieces_keep_dead_channels_the_reference_s).  fp16: a column of subnormals (2^-24) is alive, a zero column dead.
    bf16: a column 2^-45 down is alive, one at 1e-30 (its squares vanish in fp32 too) and a zero column are dead."""
    import torch
    t, k = 512, 300
    x = np.random.default_rng(5).standard_normal((t, k)).astype(np.float32)
    if dtype == "float16":
        x[:, 3] = np.where(x[:, 3] < 0, -1.0, 1.0) * np.float32(2.0 ** -24)
        x[:, 4] = 0
        live, dead = [3], [4]
    else:
        x[:, 3] *= np.float32(2.0 ** -45)
        x[:, 4] = 0
        x[:, 5] *= np.float32(1e-30)
        live, dead = [3], [4, 5]
    xd, _ = half_of(x, dtype)
    xd = xd.reshape(4, t // 4, k)
    h = torch.zeros((k, k), device="cuda")
    ops.hessian_accumulate(xd, h, 0)
    h32 = torch.zeros((k, k), device="cuda")
    ops.hessian_accumulate(xd.float(), h32, 0, method="f32")
    d, d32 = torch.diagonal(h).cpu().numpy(), torch.diagonal(h32).cpu().numpy()
    for c in live:
        assert d[c] > 0 and d32[c] > 0
    for c in dead:
        assert d[c] == 0 and d32[c] == 0
    np.testing.assert_array_equal(d == 0, d32 == 0)


# ------------------------------------------------------------------------------------ 4. method and dtype handling
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_method_is_ignored_for_half_inputs_and_kept_for_fp32(ops, restore_hessian_method, dtype):
    import torch
    x = torch.randn((4, 512, 1024), device="cuda").to(tdtype(dtype))
    outs = {}
    for m in ("auto", "f32"):
        ops.hessian_set_method(m)
        outs[m] = torch.zeros((1024, 1024), device="cuda")
        ops.hessian_accumulate(x, outs[m], 0)
    assert torch.equal(outs["auto"], outs["f32"])
    by_argument = torch.zeros((1024, 1024), device="cuda")
    ops.hessian_accumulate(x, by_argument, 0, method="bf16x9")
    assert torch.equal(by_argument, outs["auto"])
    with pytest.raises(ValueError, match="unknown Hessian method"):
        ops.hessian_accumulate(x, by_argument, 0, method="f64")
    # an fp32 input under the same thread default still takes the fp32 kernel
    ops.hessian_set_method("f32")
    x32 = x.float()
    got, f32, pieces = (torch.zeros((1024, 1024), device="cuda") for _ in range(3))
    ops.hessian_accumulate(x32, got, 0)
    ops.hessian_accumulate(x32, f32, 0, method="f32")
    ops.hessian_accumulate(x32, pieces, 0, method="f16x3")
    assert torch.equal(got, f32) and not torch.equal(got, pieces)
    # many: half items go one by one through the same kernel, fp32 items as before
    ops.hessian_set_method("auto")
    hs = [torch.zeros((1024, 1024), device="cuda") for _ in range(2)]
    assert ops.hessian_accumulate_many([x, x32], hs, [0, 0]) == [4, 4]
    assert torch.equal(hs[0], outs["auto"])
    np.testing.assert_allclose(hs[1].cpu().numpy(), outs["auto"].cpu().numpy(), rtol=0, atol=1e-5 * float(outs["auto"].abs().max()))


# ------------------------------------------------------------------------------------ 5. library errors
def test_library_errors_leave_h_untouched(ops):
    import torch
    from onnx_quantize_amd.hip import _lib as L
    lib = L.load()
    t, k = 64, 40
    x = torch.randn((t, k), device="cuda").half()
    h = torch.full((k, k), 3.0, device="cuda")
    need = lib.oq_hessian_half_workspace_bytes(t, k)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = lambda xtype, nbytes: (C.c_void_p(x.data_ptr()), xtype, t, k, k, 0, 1, C.c_void_p(h.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, stream)   # noqa: E731
    assert lib.oq_hessian_accumulate_h16(*args(L.OQ_W_F16, 1024)) == L.OQ_ERR_WORKSPACE
    assert "workspace" in lib.oq_last_error().decode()
    assert lib.oq_hessian_accumulate_h16(*args(7, need)) == L.OQ_ERR_INVALID_ARGUMENT
    assert "xtype" in lib.oq_last_error().decode()
    torch.cuda.synchronize()
    assert bool((h == 3.0).all())
    assert lib.oq_hessian_accumulate_h16(*args(L.OQ_W_F16, need)) == 0      # and the same call with what the query asks for runs
    torch.cuda.synchronize()
    assert not bool((h == 3.0).any())


# ------------------------------------------------------------------------------------ 6. driver
def test_the_driver_feeds_half_activations_as_they_are(ops):
    import torch
    from onnx_quantize_amd.calibration_driver import ActivationStream
    rng = np.random.default_rng(6)
    batches = [torch.from_numpy(rng.standard_normal((4, 64, 256)).astype(np.float32)).cuda().half() for _ in range(2)]
    stream = ActivationStream(hessian_names=["a"])
    for b in batches:
        stream.feed({"a": b, "other": b})
    torch.cuda.synchronize()
    acc = stream.hessians["a"]
    assert acc.n == 8 and "other" not in stream.hessians
    h = torch.zeros((256, 256), device="cuda")
    n = 0
    for b in batches:
        n = ops.hessian_accumulate(b, h, n)
    assert torch.equal(acc.h, h)
    x64 = torch.cat(batches).double().cpu().numpy().reshape(-1, 256)
    ref = (2.0 / 8) * x64.T @ x64
    np.testing.assert_allclose(acc.h.cpu().numpy(), ref, rtol=0, atol=1e-5 * float(np.abs(ref).max()))


# ------------------------------------------------------------------------------------ 7. / 8. files
def _nbits_arrays(model, node):
    from onnx_quantize_amd.onnx_proto import tensor_to_numpy
    inits = {t.name: t for t in model.graph.initializer}
    return tuple(tensor_to_numpy(inits[node.input[i]]) for i in (1, 2, 3))


def _dequantized(model, node, K, N, g):
    """[K, N] float64 of a uint4 MatMulNBits node: (q - zp) * scale with the scales as stored."""
    blob, s, zb = _nbits_arrays(model, node)
    blocks = K // g
    blob = blob.reshape(N, blocks, g // 2)
    q = np.stack([blob & 0x0F, blob >> 4], axis=-1).reshape(N, blocks, g).astype(np.float64)
    zb = zb.reshape(N, -1)
    z = np.stack([zb & 0x0F, zb >> 4], axis=-1).reshape(N, -1)[:, :blocks].astype(np.float64)
    return ((q - z[:, :, None]) * s.reshape(N, blocks).astype(np.float64)[:, :, None]).reshape(N, K).T


def test_file_parity_mode_matches_the_fp32_twin():
    """A two-MatMul FLOAT16 chain, GPTQ as the reference's loop is written: nothing of the Hessian's arithmetic reaches the file, so
    B and the zero points are those of the fp32 twin (weights upcast to FLOAT, FLOAT input, the upcast calibration data) and the
    scales its scales rounded to fp16."""
    from half_model_helpers import half_model
    from onnx_quantize_amd import GPTQConfig, QConfig, QuantType, QWeightArgs, quantize
    from onnx_quantize_amd.onnx_proto import DataType, parse_model, serialize

    rng = np.random.default_rng(17)
    ws = [(rng.standard_normal((64, 128)) * 0.2).astype(np.float16), (rng.standard_normal((128, 64)) * 0.2).astype(np.float16)]
    data = rng.standard_normal((8, 16, 64)).astype(np.float16)                 # 8 samples, no dead channel
    qc = lambda d: QConfig(weights=QWeightArgs(dtype=QuantType.QUInt4, group_size=32, strategy="group", algorithm=GPTQConfig(block_size=32)),   # noqa: E731
                           calibration_data=d)
    half = parse_model(quantize(serialize(half_model(ws)), qc(data), half_weights="native_calibrated"))
    twin = parse_model(quantize(serialize(half_model([w.astype(np.float32) for w in ws])), qc(data.astype(np.float32))))
    assert [n.op_type for n in half.graph.node] == ["MatMulNBits", "MatMulNBits"] == [n.op_type for n in twin.graph.node]
    for nh, nt in zip(half.graph.node, twin.graph.node):
        bh, sh, zh = _nbits_arrays(half, nh)
        bt, st, zt = _nbits_arrays(twin, nt)
        assert bh.tobytes() == bt.tobytes(), nh.name
        assert zh.tobytes() == zt.tobytes(), nh.name
        assert sh.dtype == np.float16 and st.dtype == np.float32
        assert sh.tobytes() == st.astype(np.float16).tobytes(), nh.name
    assert {t.name: t for t in half.graph.initializer}[half.graph.node[0].input[2]].data_type == DataType.FLOAT16


CORRECTED_SEED = 23


def _corrected_case(seed):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((256, 64)) * 0.2).astype(np.float16)
    mix = rng.standard_normal((16, 256))
    x = rng.standard_normal((8 * 16, 16)) @ mix                                # correlated rows: a rank-16 mix ...
    x = x / np.abs(x).std() + 0.1 * rng.standard_normal((8 * 16, 256))         # ... plus 10 % noise
    return w, x.reshape(8, 16, 256).astype(np.float16)


def _output_error(model, w, x):
    x64 = x.astype(np.float64).reshape(-1, 256)
    return float(np.linalg.norm(x64 @ w.astype(np.float64) - x64 @ _dequantized(model, model.graph.node[0], 256, 64, 32)))


def test_file_corrected_mode_is_the_composition_and_beats_rtn(ops):
    """`GPTQConfig(mode="corrected")` on a FLOAT16 file: B, scales and zero points are those of `ops.hessian_accumulate` on the
    fp16 calibration rows followed by `ops.gptq_quantize` on `w.float()`, and the output error on those rows is no larger than the
    `"native"` RTN file's.  (The fp32 twin satisfies the second condition with this seed too: checked below, first.)"""
    import torch
    from half_model_helpers import half_model
    from onnx_quantize_amd import GPTQConfig, QConfig, QuantType, QWeightArgs, quantize
    from onnx_quantize_amd.onnx_proto import parse_model, serialize

    w, x = _corrected_case(CORRECTED_SEED)
    weights = lambda algo=None: QWeightArgs(dtype=QuantType.QUInt4, group_size=32, strategy="group", **({"algorithm": algo} if algo else {}))   # noqa: E731
    gptq = lambda d: QConfig(weights=weights(GPTQConfig(block_size=32, mode="corrected")), calibration_data=d)      # noqa: E731

    w32, x32 = w.astype(np.float32), x.astype(np.float32)
    twin_gptq = parse_model(quantize(serialize(half_model([w32])), gptq(x32)))
    twin_rtn = parse_model(quantize(serialize(half_model([w32])), QConfig(weights=weights())))
    e_twin_gptq, e_twin_rtn = _output_error(twin_gptq, w, x), _output_error(twin_rtn, w, x)
    print(f"fp32 twin: ||XW - XW^|| GPTQ corrected {e_twin_gptq:.4f}, RTN {e_twin_rtn:.4f}")
    assert e_twin_gptq <= e_twin_rtn

    src = serialize(half_model([w]))
    half_gptq = parse_model(quantize(src, gptq(x), half_weights="native_calibrated"))
    half_rtn = parse_model(quantize(src, QConfig(weights=weights()), half_weights="native"))
    assert [n.op_type for n in half_gptq.graph.node] == ["MatMulNBits"]
    blob, scales, zps = _nbits_arrays(half_gptq, half_gptq.graph.node[0])

    xd, wd = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    h = torch.zeros((256, 256), device="cuda")
    assert ops.hessian_accumulate(xd, h, 0) == 8
    shared = ops.gptq_shared_factor(h, 0.01, False)
    q, s, z, info = ops.gptq_quantize(wd.float(), h, "uint4", "group", 32, block_size=32, percdamp=0.01, mode="corrected", shared=shared)
    assert int(info.item()) == 0
    assert blob.tobytes() == ops.pack_matmul_nbits(q, 32, 4).cpu().numpy().tobytes()
    assert zps.tobytes() == ops.pack_zero_points_u4(z.reshape(-1), 64, 8).cpu().numpy().tobytes()
    assert scales.dtype == np.float16
    assert scales.tobytes() == s.cpu().numpy().astype(np.float16).reshape(64, 8).tobytes()

    e_gptq, e_rtn = _output_error(half_gptq, w, x), _output_error(half_rtn, w, x)
    print(f"FLOAT16 file: ||XW - XW^|| GPTQ corrected {e_gptq:.4f}, RTN {e_rtn:.4f}")
    assert e_gptq <= e_rtn
