"""The MSE range search straight from fp16 / bf16 weights (oq_rtn_mse_h16, csrc/rtn_mse.hip).

Both conversions to fp32 are exact and the search arithmetic stays fp32, so `rtn_quantize(w_half, mse=True)` is DEFINED as
`rtn_quantize(w_half.float(), mse=True)`: the integers, the zero points and the fp32 scales are compared as raw bytes (NaN
patterns count) on every route -- the plain kernel (groups of 16, 48, 512, channels), the register tile (32 / 64 / 128), the packed
tile (256), the tensor route -- through views with a leading dimension and rows that are only 2-byte aligned.  One case per
element type goes straight against the oracle through tests/mse_verdict.py, and the calls must not allocate an fp32 copy."""
import ctypes as C

import numpy as np
import pytest

import mse_half_cases as M
import mse_verdict as V
import oq_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = ["float16", "bfloat16"]
QTYPES = ["uint4", "int4", "uint8", "int8"]


def _same(a, b):
    """q, scale and zero point of two `rtn_quantize` results, bit for bit."""
    import torch
    if (a[0] is None) != (b[0] is None):
        return False
    if a[0] is not None and not (a[0].dtype == b[0].dtype and a[0].shape == b[0].shape and torch.equal(a[0], b[0])):
        return False
    return (a[1].dtype == b[1].dtype == torch.float32 and a[1].shape == b[1].shape and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
            and a[2].dtype == b[2].dtype and a[2].shape == b[2].shape and torch.equal(a[2], b[2]))


def _check(ops, w, qtype, strategy, g, sym=False, red=False, what=None, **kw):
    """The half call against the fp32 route on the upcast matrix; returns the half call's result."""
    import torch
    assert w.dtype in (torch.float16, torch.bfloat16)
    got = ops.rtn_quantize(w, qtype, strategy, g, sym, red, 1.0, True, **kw)
    ref = ops.rtn_quantize(w.float(), qtype, strategy, g, sym, red, 1.0, True, **kw)
    assert _same(got, ref), (what, str(w.dtype), tuple(w.shape), qtype, strategy, g, sym, red, kw)
    return got


@pytest.fixture(scope="module")
def ops():
    from onnx_quantize_amd.hip import ops as _ops
    return _ops


_BASES = {}


def _bases(dtype):
    """The base matrices of one element type, made once: 512 x 600, a 601-wide one for rows that are only 2-byte aligned, and a
    1024 x 300 one for groups of 512 and channels of 513 rows.  Column-scaled: every column has its own range."""
    import torch
    if dtype not in _BASES:
        gen = torch.Generator(device="cuda").manual_seed(180 + len(dtype))
        dt = getattr(torch, dtype)
        make = lambda k, n: (torch.randn((k, n), generator=gen, device="cuda") * (0.5 + torch.rand(n, generator=gen, device="cuda"))).to(dt)  # noqa: E731
        _BASES[dtype] = (make(512, 600), make(512, 601), make(1024, 300))
    return _BASES[dtype]


# ------------------------------------------------------------------------------------ every route at its smallest shape
@pytest.mark.parametrize("g", [16, 48, 32, 64, 128, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_half_weights_give_the_fp32_route_s_bits(ops, dtype, g):
    """16 and 48: the plain kernel; 32 / 64 / 128: the register tile; 256: the packed tile."""
    import torch
    big, odd, _ = _bases(dtype)
    k2, k1 = 512 // g * g, 256 // g * g                                         # 512 and 256 rows, 480 and 240 at g = 48
    unaligned = odd[2:2 + k1, 3:136]                      # ldw 601, first element 1205: every other row starts on an odd element
    assert unaligned.data_ptr() % 4 == 2 and unaligned.stride(0) % 2 == 1
    views = (big[:k2, :520], big[:k1, 8:140], unaligned, big[:g, :520])         # ldw 600, N % 256 != 0; ragged; odd; K = g: one group
    for i, w in enumerate(views):
        assert w.dtype == getattr(torch, dtype) and not w.is_contiguous()
        q, s, z = _check(ops, w, "uint4", "group", g, what=f"view {i}")
        assert q.shape == w.shape and s.shape == (w.numel() // g, 1) and bool(torch.isfinite(s).all())
        _check(ops, w, "int4", "group", g, True, what=f"view {i} sym")
    # the search really searched: some rows left candidate 0 (their scale is below the plain RTN one)
    s_mse = ops.rtn_quantize(views[0], "uint4", "group", g, mse=True)[1]
    s_rtn = ops.rtn_quantize(views[0], "uint4", "group", g)[1]
    assert bool((s_mse < s_rtn).any()) and bool((s_mse <= s_rtn * (1 + 1e-6)).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_groups_above_the_tiles_channels_and_the_tensor_route(ops, dtype):
    """g = 512 on 1024 rows (the plain kernel above the tiles), channels of 33 and 513 rows, the tensor route on 200 x 72 and 1 x 5."""
    tall = _bases(dtype)[2]
    _check(ops, tall[:, 5:269], "uint4", "group", 512, what="g512")
    _check(ops, tall[:, 5:269], "int8", "group", 512, True, what="g512 int8 sym")
    for k in (33, 513):
        _check(ops, tall[:k, 3:263], "uint4", "channel", -1, what=f"channel {k}")
        _check(ops, tall[1:1 + k, 3:263], "int8", "channel", -1, True, what=f"channel {k} int8 sym, odd base")
    for view in (tall[:200, 7:79], tall[9:10, 11:16], tall[:200, :72].contiguous()):
        for qtype, sym in (("uint4", False), ("int4", True), ("uint8", False), ("int8", True)):
            q, s, z = _check(ops, view, qtype, "tensor", -1, sym, what="tensor")
            assert s.shape == () and z.shape == ()


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("g", [128, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_widths_around_a_block(ops, dtype, g, n):
    """N = 1, 255, 257: the tail lanes of the last block load a clamped address and store nothing."""
    big, odd, _ = _bases(dtype)
    _check(ops, big[:, 7:7 + n], "uint4", "group", g, what=f"N {n}")
    _check(ops, odd[:, 300:300 + n], "uint4", "group", g, what=f"N {n}, odd ldw")
    _check(ops, big[:, 7:7 + n].contiguous(), "int4", "group", g, True, what=f"N {n} contiguous")


@pytest.mark.parametrize("g", [64, 256])
@pytest.mark.parametrize("qtype", QTYPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_types_and_flags(ops, dtype, qtype, g):
    """Every quantization type x symmetric x reduce_range; parameters only; the caller's buffers."""
    import torch
    w = _bases(dtype)[0][:, 8:300]
    for sym in (False, True):
        for red in (False, True):
            got = _check(ops, w, qtype, "group", g, sym, red)
            only = _check(ops, w, qtype, "group", g, sym, red, emit_q=False)
            assert only[0] is None and _same((None, got[1], got[2]), only)
    count = w.numel() // g
    cdt = ops.container_dtype(qtype)
    out = (torch.full(tuple(w.shape), 0x5A, dtype=cdt, device="cuda"), torch.full((count,), -7.0, device="cuda"),
           torch.full((count,), 0x5A, dtype=cdt, device="cuda"))
    ptrs = [t.data_ptr() for t in out]
    res = ops.rtn_quantize(w, qtype, "group", g, mse=True, out=out)
    assert [res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr()] == ptrs
    assert _same(res, ops.rtn_quantize(w.float(), qtype, "group", g, mse=True))


# ------------------------------------------------------------------------------------ special values
SPECIALS = {"float16": (65504.0, -65504.0, 2.0 ** -24, 0.0, -0.0), "bfloat16": (3.39e38, -3.39e38, 2.0 ** -133, 0.0, -0.0)}


@pytest.mark.parametrize("g", [64, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values_and_nan(ops, dtype, g):
    """The largest finite values, a subnormal and both zeros in the first, a middle and the last row of a group; then a NaN, which
    changes its own row's parameters and, through the global stop, nothing the fp32 route does not change either: equality with
    the fp32 route is the assertion."""
    import torch
    dt = getattr(torch, dtype)
    clean = _bases(dtype)[0][:, :300].clone()
    w = clean.clone()
    col = 0
    for row in (0, g // 2 - 1, g - 1):                   # of group 0, and the same rows of the last group
        for value in SPECIALS[dtype]:
            w[row, col] = value
            w[512 - g + row, col + 150] = value
            col += 1
    assert torch.isfinite(w.float()).all() and (w.float() != 0).sum() < w.numel()
    sub = torch.tensor(SPECIALS[dtype][2], dtype=dt)
    assert float(sub) == SPECIALS[dtype][2] and 0 < float(sub) < float(torch.finfo(dt).tiny)        # a subnormal of the type
    for qtype, sym in (("uint4", False), ("int4", True), ("uint8", False)):
        _check(ops, w, qtype, "group", g, sym, what="specials")
    poisoned = clean.clone()
    poisoned[g + 3, 7] = float("nan")                    # group 1 of column 7
    got = _check(ops, poisoned, "uint4", "group", g, what="nan")
    s = got[1].reshape(300, 512 // g)
    assert bool(torch.isnan(s[7, 1])) and int(torch.isnan(s).sum()) == 1
    _check(ops, poisoned, "uint4", "channel", -1, what="nan channel")
    _check(ops, poisoned, "uint4", "tensor", -1, what="nan tensor")


@pytest.mark.parametrize("g", [128, 256])
def test_tiny_and_ordinary_columns_in_one_wave_bf16(ops, g):
    """Odd columns around 1e-15, even columns ordinary: every wave holds rows whose unshrunk scale is below 2^-32 (the shifted
    power path of csrc/rtn_mse.hip, wave-uniform) next to rows that take it with a shift of 0.
    bf16 only: fp16 cannot produce such a scale -- its smallest non-zero range is the subnormal 2^-24, over at most 255 levels that
    is 2^-24 / 255 > 2^-32."""
    import torch
    w32 = torch.from_numpy(np.random.default_rng(4).standard_normal((2 * g, 320), dtype=np.float32)).cuda()
    w32[:, 1::2] *= 1e-15
    w = w32.to(torch.bfloat16)
    q, s, z = _check(ops, w, "uint4", "group", g, what="mixed wave")
    s = s.reshape(320, 2)
    assert bool((s[1::2] < 2.0 ** -32).all()) and bool((s[0::2] > 2.0 ** -10).all())
    _check(ops, w[:, 1:], "int4", "group", g, True, what="mixed wave sym, odd base")


# ------------------------------------------------------------------------------------ the stop rule
@pytest.mark.parametrize("dtype", DTYPES)
def test_early_stop_inside_the_walk(ops, dtype):
    """The matrix of test_mse_stop_strictly_inside_the_walk (64 x 32, seed 36, uint4 g = 16: the oracle stops at 13 on the fp32
    values) after a round trip through the element type: the fp32 route's bits, and rows that left candidate 0."""
    import torch
    w = torch.from_numpy(np.random.default_rng(36).standard_normal((64, 32), dtype=np.float32)).cuda().to(getattr(torch, dtype))
    _, s, _ = _check(ops, w, "uint4", "group", 16, what="early stop")
    s0 = ops.rtn_quantize(w, "uint4", "group", 16)[1]
    assert bool((s != s0).any()), "every row sits on candidate 0"
    for g in (32, 64):                                                           # the same walk on the register tile
        _check(ops, w, "uint4", "group", g, what="early stop")


# ------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("g", M.ORACLE_GROUPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_half_weights_against_the_oracle(ops, dtype, g):
    """256 x 192, uint4, the oracle on the upcast matrix through tests/mse_verdict.py, as `run_case` of tests/test_mse_gpu.py
    does: rows the reference decides by more than 2 tau equal it bit for bit, the others (at most 1 %: asserted on the CPU in
    tests/test_mse_half_abi.py for this very input) stay within 2 tau of the best."""
    import torch
    w = M.oracle_matrix(dtype)
    undecided, rows, t, j = M.undecided_rows(w, g)
    assert undecided <= rows // 100
    assert j.stop == V.oracle_stop(w, "uint4", "group", g, False, False, t), "the tables' stop is not the oracle's"
    eq, es, ez = O.rtn_quantize(w, "uint4", "group", g, False, False, 1.0, True)
    wd = torch.from_numpy(w).cuda().to(getattr(torch, dtype))
    assert torch.equal(wd.float().cpu(), torch.from_numpy(w))                    # the device holds exactly the oracle's values
    q, s, z = ops.rtn_quantize(wd, "uint4", "group", g, mse=True)
    q, s, z = q.cpu().numpy(), s.cpu().numpy(), z.cpu().numpy()
    assert q.shape == eq.shape and q.dtype == eq.dtype and z.dtype == ez.dtype and s.shape == es.shape and z.shape == ez.shape
    x_rows = V.rows_of(w, "group", g)
    what = f"{dtype} g{g}"
    v = V.verdict(t, j, s, z, es, ez, V.rows_of(q, "group", g), V.rows_of(eq, "group", g), what,
                  requantize=lambda row, sc, zp: O.quantize(x_rows[row], sc, int(zp), "uint4", False, False))
    if j.stop_decided:                                                           # no row may sit on a candidate after the stop
        on_grid_before = np.zeros(rows, bool)
        sg, zg = s.reshape(-1), z.reshape(-1).astype(np.int64)
        for i in range(j.stop + 1):
            on_grid_before |= (t.scales[i].view(np.uint32) == sg.view(np.uint32)) & (t.zps[i] == zg)
        assert np.all(on_grid_before | t.nan_rows), f"{what}: a row ended after the stop iteration {j.stop}"
    print(f"[mse half] {what}: rows {v.rows} undecided {v.undecided} differing {v.differing} stop {v.stop} tau {v.tau:.3g}")
    assert v.undecided <= rows // 100


# ------------------------------------------------------------------------------------ no fp32 copy
def _rise(call):
    """Bytes the allocated memory rises by during `call`, after a warm call (the HQQ workspace is kept from it)."""
    import torch
    out = call()
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = call()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before, out


@pytest.mark.parametrize("g", [128, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_fp32_copy_of_the_weight_is_made(ops, dtype, g):
    """The rise of the allocated bytes during a call covers q (a byte per element), the parameters and the search's rows (12
    bytes per group); an fp32 copy alone would be four bytes per element."""
    import torch
    w = (torch.randn((2048, 2048), device="cuda") * 0.1).to(getattr(torch, dtype))
    rise, out = _rise(lambda: ops.rtn_quantize(w, "uint4", "group", g, mse=True))
    assert out[0].shape == (2048, 2048)
    assert rise < 2 * w.numel(), (rise, w.numel())
    del out
    rise, out = _rise(lambda: ops.hqq_quantize(w, g, mse=True))
    assert out[0].shape == (2048, 2048)
    assert rise < 2 * w.numel(), (rise, w.numel())


@pytest.mark.parametrize("dtype", DTYPES)
def test_hqq_with_mse_gives_the_fp32_route_s_bits(ops, dtype):
    import torch
    w = _bases(dtype)[0][:, :520]
    for g in (64, 256):
        a, b = ops.hqq_quantize(w, g, mse=True), ops.hqq_quantize(w.float(), g, mse=True)
        assert torch.equal(a[0], b[0]) and int(a[3]) == int(b[3])
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


# ------------------------------------------------------------------------------------ seam and file
class _Tensor:
    def __init__(self, a):
        self._a = a

    def numpy(self):
        return self._a


class _Value:
    def __init__(self, name, const_value=None):
        self.name, self.const_value = name, const_value


@pytest.mark.parametrize("g", [32, 256])
@pytest.mark.parametrize("flagged", [False, True], ids=["plain", "matmul_nbits"])
def test_seam_takes_half_weights_with_mse(flagged, g):
    """The three arrays for an np.float16 value and for resident fp16 / bf16 values: the bytes of the fp32 twin."""
    import torch
    from onnx_quantize_amd import QConfig, QuantType, QWeightArgs, seam
    w16 = np.random.default_rng(31).standard_normal((512, 64)).astype(np.float16)
    qc = QConfig(weights=QWeightArgs(dtype=QuantType.from_string("uint4"), group_size=g, strategy="group", mse=True))
    assert qc.weights.mse
    run = lambda value: seam.weight_arrays(value, qc, None, flagged)      # noqa: E731
    ref = run(_Value("fc.weight", _Tensor(w16.astype(np.float32))))
    got = run(_Value("fc.weight", _Tensor(w16)))
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    plain = seam.weight_arrays(_Value("fc.weight", _Tensor(w16)), QConfig(weights=QWeightArgs(dtype=QuantType.from_string("uint4"), group_size=g,
                                                                                              strategy="group")), None, flagged)
    assert plain[1].tobytes() != got[1].tobytes()                         # mse reached the kernels: other scales than plain RTN
    for dt in (torch.float16, torch.bfloat16):
        resident = torch.from_numpy(w16).cuda().to(dt)
        value = _Value("fc.weight", _Tensor(np.zeros((512, 64), np.float16)))
        value.device_value, value.placeholder = resident, True
        got = run(value)
        ref = run(_Value("fc.weight", _Tensor(resident.float().cpu().numpy())))
        for a, b in zip(got, ref):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_native_file_path_with_mse():
    """A FLOAT16 file through quantize(..., half_weights="native") with mse: B and the zero points of every node are byte-equal
    to those of the fp32 twin file (its scales are fp32, the native file's float16)."""
    from half_model_helpers import half_model
    from onnx_quantize_amd import QConfig, QuantType, QWeightArgs, quantize
    from onnx_quantize_amd.onnx_proto import parse_model, serialize, tensor_to_numpy
    rng = np.random.default_rng(17)
    ws = [(rng.standard_normal((64, 128)) * 0.2).astype(np.float16), (rng.standard_normal((128, 64)) * 0.2).astype(np.float16)]
    qc = lambda: QConfig(weights=QWeightArgs(dtype=QuantType.QUInt4, group_size=32, strategy="group", mse=True))      # noqa: E731
    half = parse_model(quantize(serialize(half_model(ws)), qc(), half_weights="native"))
    twin = parse_model(quantize(serialize(half_model([w.astype(np.float32) for w in ws])), qc()))
    assert [n.op_type for n in half.graph.node] == [n.op_type for n in twin.graph.node] == ["MatMulNBits", "MatMulNBits"]
    hi, ti = ({t.name: tensor_to_numpy(t) for t in m.graph.initializer} for m in (half, twin))
    for hn, tn in zip(half.graph.node, twin.graph.node):
        for slot in (1, 3):                                                      # B, zero points
            a, b = hi[hn.input[slot]], ti[tn.input[slot]]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        assert hi[hn.input[2]].dtype == np.float16 and ti[tn.input[2]].dtype == np.float32
        assert hi[hn.input[2]].tobytes() == ti[tn.input[2]].astype(np.float16).tobytes()


# ------------------------------------------------------------------------------------ refusals
def test_refusals(ops):
    import torch
    from onnx_quantize_amd.hip import _lib as L
    w = torch.randn((256, 64), device="cuda").to(torch.float16)
    # through ops: what raised before the half route existed raises the same
    with pytest.raises(Exception, match="NBITS layout with mse is not supported"):
        ops.rtn_quantize(w, "uint4", "group", 128, mse=True, layout="nbits")
    with pytest.raises(Exception, match="KN_PACKED4 layout needs .* no mse"):
        ops.rtn_quantize(w, "uint4", "group", 128, mse=True, layout="kn_packed4")
    with pytest.raises(Exception, match="mse with groups that straddle columns"):
        ops.rtn_quantize(w[:96], "uint4", "group", 64, mse=True)           # 96 * 64 % 64 == 0 but K % g != 0
    with pytest.raises(TypeError):
        ops.rtn_quantize(torch.zeros((64, 64), dtype=torch.float16), "uint4", "group", 32, mse=True)      # a CPU tensor: no fallback
    # through the library: the status, the message, and nothing written
    lib = L.load()
    k, n = 96, 64
    wb = torch.randn((k, n), device="cuda").to(torch.bfloat16)
    q = torch.full((k, n), 0xAB, dtype=torch.uint8, device="cuda")
    s = torch.full((k * n // 32,), -3.0, device="cuda")
    z = torch.full((k * n // 32,), 0xAB, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda g, layout: lib.oq_rtn_mse_h16(C.c_void_p(wb.data_ptr()), L.OQ_W_BF16, k, n, n, L.OQ_UINT4, L.OQ_GROUP, g, 0, 0, 1.0,    # noqa: E731
                                                C.c_void_p(q.data_ptr()), C.c_void_p(s.data_ptr()), C.c_void_p(z.data_ptr()), layout,
                                                C.c_void_p(ws.data_ptr()), ws.numel(), stream)
    for g, layout, word in ((32, L.OQ_LAYOUT_NBITS, "NBITS"), (32, L.OQ_LAYOUT_KN_PACKED4, "KN_PACKED4"), (64, L.OQ_LAYOUT_KN, "straddle")):
        assert call(g, layout) == L.OQ_ERR_UNSUPPORTED
        msg = lib.oq_last_error().decode()
        assert "oq_rtn_mse_h16" in msg and word in msg, msg
    torch.cuda.synchronize()
    assert bool((q == 0xAB).all()) and bool((s == -3.0).all()) and bool((z == 0xAB).all()) and not bool(ws.any())
    assert call(32, L.OQ_LAYOUT_KN) == 0, lib.oq_last_error().decode()          # the same buffers, accepted
    assert _same((q, s.reshape(-1, 1), z.reshape(-1, 1)), ops.rtn_quantize(wb.float(), "uint4", "group", 32, mse=True))
