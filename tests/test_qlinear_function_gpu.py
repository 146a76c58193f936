"""`ops.qlinear_function` / `ops.qlinear_function_decode` / `oq_qlinear_function[_decode]` (include/oq_hip_qlinear_function.h,
csrc/qlinear_function.hip): one call of a `quant`-domain QLinearMatMul / QLinearGemm function, fp32 X in and fp32 Y out.

Every comparison is of BYTES.  The oracle (qlinear_function_cases.FCase): the NumPy restatement of the quantizer, the exact int64
product of the quantized X on the CPU, `qlinear_cases.restate`, then (q - zp) * y_scale in np.float32.

1  the identity probe: B = I_K shows the quantized bytes themselves.
2  the tile route over the table of test_qlinear_matmul_gpu.py, the quantizer's edges, strides, a 512-tile grid.
3  the decode route over the rows and the table of test_qlinear_decode_gpu.py, both routes of the upper NK tiers, a 512-workgroup grid.
4  agreement: with the three nodes run one after the other by the runner's own code, and of the two routes with each other.
5  memory and refusals.
"""
import numpy as np
import pytest
import torch

from qlinear_cases import KN, LAYOUTS, NK, RANGE, SIGNS, gen
from qlinear_function_cases import F, FCase, decode_workspace, draw_x, edges, plant, quantize_np, raw_function, same_bytes, workspace
from test_qlinear_decode_gpu import ROWS, TABLE, ZPS
from test_qlinear_matmul_gpu import SWEEP

pytestmark = pytest.mark.gpu

DT = {"u8": torch.uint8, "i8": torch.int8}


@pytest.fixture(scope="module")
def ops():
    from onnx_quantize_amd.hip import ops
    return ops


@pytest.fixture(scope="module")
def lib():
    from onnx_quantize_amd.hip import _lib
    return _lib.load()


def sign_id(s):
    return f"{s[0]}x{s[1]}"


def where_wrong(got, want):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    return f"{len(bad)} of {got.size} differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"


# ------------------------------------------------------------------------------------ 1. the identity probe
@pytest.mark.parametrize("end", ["bottom", "top"])
@pytest.mark.parametrize("dt", ["u8", "i8"])
@pytest.mark.parametrize("decode", [False, True], ids=["tile", "decode"])
def test_the_identity_probe_shows_the_quantized_bytes(ops, decode, dt, end):
    """B = I_K (int8, no zero point), b_scale = 1, s = y_scale = 2^-5, y_type = a_type, y_zp = x_zp: t = acc * s exactly, t / s = acc,
    so Y / s + zp IS q_a, at no tolerance.  X: every level of the type, ties from both sides at even and odd levels, and the hostile
    values in the first, a middle and the last position and in the last partial 16-chunk."""
    fn = ops.qlinear_function_decode if decode else ops.qlinear_function
    dtype, s = DT[dt], 2.0 ** -5
    lo, hi = RANGE[dtype]
    zp = lo if end == "bottom" else hi
    scale, zero, one = torch.tensor(s, device="cuda"), torch.tensor(zp, dtype=dtype, device="cuda"), torch.tensor(1.0, device="cuda")
    rng = np.random.default_rng(7)
    for K in (1, 15, 16, 17, 64, 65, 1040):
        M = 16
        q0 = rng.integers(lo, hi + 1, (M, K))
        q0.reshape(-1)[: min(M * K, 256)] = np.arange(lo, hi + 1)[: min(M * K, 256)]          # every level where there is room
        x = plant(draw_x(rng, q0, zp, s, ties=True), edges(zp, s, dtype))
        want_q = quantize_np(x, s, zp, dtype)
        y = fn(torch.from_numpy(x).cuda(), scale, zero, torch.eye(K, dtype=torch.int8, device="cuda"), one, None, scale, zero)
        assert y.dtype == torch.float32 and y.shape == (M, K)
        got_q = y.cpu().numpy() / F(s) + F(zp)
        assert np.array_equal(got_q, want_q.astype(F)), (K, np.argwhere(got_q != want_q)[:4], got_q[got_q != want_q][:4], want_q[got_q != want_q][:4])
        assert want_q.min() == lo and want_q.max() == hi                                          # both ends are reached (saturation)


# ------------------------------------------------------------------------------------ 2. the tile route
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("signs", SIGNS, ids=sign_id)
def test_the_tile_route_over_the_table(lib, signs, layout):
    """The (M, K, N) table of the integer kernel (partial tiles; K one short of and one past a step; split K with a short last
    split) and its zero-point forms; b_scale per tensor / per column and the bias alternate along the table, y's type with the signs."""
    bad = []
    for i, (M, K, N, zp, why) in enumerate(SWEEP):
        f = FCase(gen(300 + i), 300 + i, M, K, N, signs[0], signs[1], LAYOUTS[layout], zp=zp, bias=i % 2 == 0, per_column=i % 3 != 0,
                  hostile=i % 4 == 1, y_dt=DT[signs[1]])
        st, y = raw_function(lib, f)
        assert st == 0, lib.oq_last_error().decode()
        got = y.cpu().numpy()
        if not same_bytes(got, f.want):
            bad.append(f"{(M, K, N, zp)} [{why}]: {where_wrong(got, f.want)}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("zp", ZPS)
def test_the_tile_route_with_every_zero_point_form(lib, zp):
    for signs in SIGNS:
        for bias in (False, True):
            f = FCase(gen(11), 11, 33, 200, 130, signs[0], signs[1], KN if bias else NK, zp=zp, bias=bias, per_column=bias, hostile=True)
            st, y = raw_function(lib, f)
            assert st == 0 and same_bytes(y, f.want), (signs, bias, where_wrong(y.cpu().numpy(), f.want))


@pytest.mark.parametrize("decode", [False, True], ids=["tile", "decode"])
def test_gaps_odd_bases_and_strided_views_give_the_contiguous_bytes(lib, decode):
    """lda > K with NaN and 3e38 in the gap (never read), X offset by one float (rows 4-byte aligned only), a row view with a stride
    that keeps 16-byte alignment, ldy > N with a sentinel in the gap (never written)."""
    M, K, N = 16, 77, 100
    for layout in (KN, NK):
        f = FCase(gen(21), 21, M, K, N, "u8", "i8", layout, zp="lo", bias=True, per_column=True, hostile=True)
        for lda, offset in ((K + 2, 0), (K + 2, 1), (80, 0), (K, 1)):
            buf = torch.full((M * lda + 4,), float("nan"), dtype=torch.float32, device="cuda")
            buf[1::2] = 3e38
            x = buf[offset: offset + M * lda].view(M, lda)[:, :K]
            x.copy_(f.x)
            assert x.data_ptr() % 16 == (4 * offset) % 16
            y_buf = torch.full((M, N + 5), -7.25, dtype=torch.float32, device="cuda")
            st, _ = raw_function(lib, f, decode=decode, x=x, lda=lda, y=y_buf, ldy=N + 5)
            assert st == 0, lib.oq_last_error().decode()
            assert same_bytes(y_buf[:, :N].contiguous(), f.want), (layout, lda, offset, where_wrong(y_buf[:, :N].cpu().numpy(), f.want))
            assert (y_buf[:, N:] == -7.25).all()


def test_a_512_tile_grid_four_times_over(ops):
    M, K, N = 2048, 128, 4096                      # 16 x 32 tiles of 128 x 128
    f = FCase(gen(31), 31, M, K, N, "u8", "i8", KN, zp="lo", per_column=True)
    first = f.call(ops.qlinear_function)
    assert same_bytes(first, f.want), where_wrong(first.cpu().numpy(), f.want)
    for _ in range(3):
        assert torch.equal(f.call(ops.qlinear_function).view(torch.int32), first.view(torch.int32))


# ------------------------------------------------------------------------------------ 3. the decode route
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("signs", SIGNS, ids=sign_id)
def test_the_decode_route_over_rows_and_table(lib, signs, layout):
    """Every row count at both ends of a tier against the (K, N) table of the integer decode kernel (one slice and several, a short
    last one); the zero-point forms, the bias and b_scale's form rotate along it."""
    bad = []
    for i, (K, N) in enumerate(TABLE):
        for j, M in enumerate(ROWS):
            zp = ZPS[(i + j) % len(ZPS)]
            f = FCase(gen(500 + i), 500 + 16 * i + j, M, K, N, signs[0], signs[1], LAYOUTS[layout], zp=zp, bias=(i + j) % 2 == 0,
                      per_column=(i + j) % 3 != 0, hostile=j % 2 == 1, y_dt=DT[signs[0]])
            st, y = raw_function(lib, f, decode=True)
            assert st == 0, lib.oq_last_error().decode()
            if not same_bytes(y, f.want):
                bad.append(f"{(M, K, N, zp)}: {where_wrong(y.cpu().numpy(), f.want)}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("signs", SIGNS, ids=sign_id)
def test_both_routes_of_the_upper_tiers_of_an_nk_matrix(lib, signs):
    """M = 5 ... 16 against an NK matrix with 16-byte aligned rows and K a multiple of 16 runs on the matrix cores; the same operands
    with B one byte off an alignment keep dot4.  Several slices with a short last one (K = 2064), then K no multiple of 16."""
    for M in (5, 8, 9, 16):
        f = FCase(gen(41), 41 + M, M, 2064, 70, signs[0], signs[1], NK, zp="lo", bias=True, per_column=True, hostile=True)
        st, y = raw_function(lib, f, decode=True)
        assert st == 0 and same_bytes(y, f.want), (M, where_wrong(y.cpu().numpy(), f.want))
        aligned = f.c.b
        odd = torch.empty(aligned.numel() + 16, dtype=aligned.dtype, device="cuda")[1: 1 + aligned.numel()].view_as(aligned)
        odd.copy_(aligned)
        f.c.b = odd
        st, y = raw_function(lib, f, decode=True)
        f.c.b = aligned
        assert st == 0 and same_bytes(y, f.want), (M, "dot4", where_wrong(y.cpu().numpy(), f.want))
        g = FCase(gen(43), 43 + M, M, 2050, 70, signs[0], signs[1], NK, zp="hi", hostile=True)
        st, y = raw_function(lib, g, decode=True)
        assert st == 0 and same_bytes(y, g.want), (M, "K = 2050", where_wrong(y.cpu().numpy(), g.want))


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("M", [1, 16])
def test_a_512_workgroup_decode_grid_four_times_over(ops, M, layout):
    from qlinear_decode_cases import plan
    K, N = (2048, 4096) if layout == "NK" else (1024, 8192)
    assert plan(M, K, N, LAYOUTS[layout]).grid >= 256
    f = FCase(gen(51), 51, M, K, N, "u8", "i8", LAYOUTS[layout], zp="lo", per_column=True)
    first = f.call(ops.qlinear_function_decode)
    assert same_bytes(first, f.want), where_wrong(first.cpu().numpy(), f.want)
    for _ in range(3):
        assert torch.equal(f.call(ops.qlinear_function_decode).view(torch.int32), first.view(torch.int32))


# ------------------------------------------------------------------------------------ 4. agreement
def composition(ops, f, x):
    """What the runner executes under "fused": its own `_quantize`, `ops.qlinear_matmul` with an 8-bit output, its own
    `_op_DequantizeLinear`."""
    from onnx_quantize_amd.graph_runner import GraphRunner, _Attrs
    runner = GraphRunner.evaluator(21)
    c = f.c
    q = runner._quantize(x, f.a_scale, c.a_zp)
    out = ops.qlinear_matmul(q, f.a_scale, c.a_zp, c.b, f.b_scale, c.b_zp, f.y_scale, f.y_zp, bias=c.bias, trans_b=c.trans_b)
    return runner._op_DequantizeLinear(None, [out, f.y_scale, f.y_zp], _Attrs({}), None)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("dt", ["u8", "i8"])
def test_one_call_has_the_bytes_of_the_three_nodes_and_the_routes_agree(ops, dt, layout):
    """Inputs without NaN (torch's cast of one is undefined): ties at a power-of-two scale and every other hostile value included."""
    for M, K, N in ((16, 200, 130), (5, 1088, 100), (33, 65, 260)):
        for scale, ties in ((0.0123, False), (2.0 ** -6, True)):
            f = FCase(gen(61), 61, M, K, N, dt, "i8", LAYOUTS[layout], zp="lo", bias=True, per_column=True, scale=scale, ties=ties, y_dt=DT[dt])
            za = int(f.c.a_zp)
            x = plant(f.x_np.copy(), edges(za, scale, DT[dt])[:-1])                     # all but the NaN
            x_dev = torch.from_numpy(x).cuda()
            one = ops.qlinear_function(*f.args(x_dev), bias=f.c.bias, trans_b=f.c.trans_b)
            three = composition(ops, f, x_dev)
            assert one.dtype == three.dtype == torch.float32
            assert torch.equal(one.view(torch.int32), three.view(torch.int32)), (M, K, N, scale, where_wrong(one.cpu().numpy(), three.cpu().numpy()))
            if M <= 16:
                dec = ops.qlinear_function_decode(*f.args(x_dev), bias=f.c.bias, trans_b=f.c.trans_b)
                assert torch.equal(dec.view(torch.int32), one.view(torch.int32))


def test_leading_axes_are_flattened_and_restored_and_an_empty_input_returns_empty(ops):
    f = FCase(gen(71), 71, 12, 96, 40, "u8", "i8", KN, zp="lo")
    for fn in (ops.qlinear_function, ops.qlinear_function_decode):
        y = f.call(fn, f.x.reshape(2, 3, 2, 96))
        assert y.shape == (2, 3, 2, 40) and same_bytes(y.reshape(12, 40), f.want)
        empty = f.call(fn, f.x[:0].reshape(0, 3, 96))
        assert empty.shape == (0, 3, 40) and empty.dtype == torch.float32


# ------------------------------------------------------------------------------------ 5. memory and refusals
def test_peak_memory_of_a_call_is_the_output_and_the_workspace(ops, lib):
    M, K, N = 16, 1024, 1024
    f = FCase(gen(81), 81, M, K, N, "u8", "i8", KN, zp="mid")
    r512 = lambda n: (n + 511) // 512 * 512      # noqa: E731  (the allocator's granule)

    def growth(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        del out
        return peak

    for fn, need in ((ops.qlinear_function, lib.oq_qlinear_function_workspace_bytes(M, K, N)),
                     (ops.qlinear_function_decode, lib.oq_qlinear_function_decode_workspace_bytes(M, K, N, KN))):
        f.call(fn)
        assert need == (workspace(M, K, N) if fn is ops.qlinear_function else decode_workspace(M, K, N, KN))
        assert growth(lambda: f.call(fn)) == r512(M * N * 4) + (r512(max(need, 256)) if need or fn is ops.qlinear_function else 0)


def test_refusals_leave_y_untouched_and_the_op_raises_by_name(ops, lib):
    f = FCase(gen(91), 91, 8, 64, 16, "u8", "i8", KN, zp="mid")
    y = torch.full((8, 16), 99.0, dtype=torch.float32, device="cuda")
    for decode in (False, True):
        name = "oq_qlinear_function_decode" if decode else "oq_qlinear_function"
        for kw, status, word in ((dict(flags=1), -2, "per-row"), (dict(flags=2), -2, "transA"), (dict(flags=4), -2, "alpha"),
                                 (dict(a_code=5), -1, "a_type"), (dict(b_code=5), -1, "b_type"), (dict(layout=7), -1, "b_layout"),
                                 (dict(y_code=2), -1, "y_type"), (dict(ldy=15), -1, "ldy=15"), (dict(lda=63), -1, "lda=63")):
            st, _ = raw_function(lib, f, decode=decode, y=y, **{"ldy": 16, **kw})
            msg = lib.oq_last_error().decode()
            assert st == status and word in msg and name in msg, (kw, st, msg)
    st = lib.oq_qlinear_function_decode(f.x.data_ptr(), 0, 17, 64, 64, f.a_scale.data_ptr(), None, f.c.b.data_ptr(), 1, KN, 16, 16,
                                        f.b_scale.data_ptr(), None, 0, None, f.y_scale.data_ptr(), None, 0, 0, y.data_ptr(), 16, None, 0, None)
    assert st == -2 and "M = 17 rows" in lib.oq_last_error().decode()
    torch.cuda.synchronize()
    assert (y == 99.0).all()

    wide = torch.zeros((17, 64), dtype=torch.float32, device="cuda")
    with pytest.raises(NotImplementedError, match="17 rows"):
        f.call(ops.qlinear_function_decode, wide)
    assert f.call(ops.qlinear_function, wide).shape == (17, 16)
    for fn in (ops.qlinear_function, ops.qlinear_function_decode):
        with pytest.raises(NotImplementedError, match="fp32 has a kernel"):
            f.call(fn, f.x.half())
        with pytest.raises(NotImplementedError, match="per-row a_scale"):
            fn(f.x, torch.full((8,), 0.02, device="cuda"), *f.args()[2:])
        with pytest.raises(NotImplementedError, match="not fp32"):
            fn(f.x, f.a_scale.half(), *f.args()[2:])
        with pytest.raises(TypeError, match="GPU memory"):
            f.call(fn, f.x.cpu())
    assert ops.qlinear_function_unsupported(*f.args()) is None and ops.qlinear_function_decode_unsupported(*f.args()) is None
    assert "17 rows" in ops.qlinear_function_decode_unsupported(wide, *f.args()[1:])
    assert "out_scale" in ops.qlinear_function_unsupported(*f.args()[:6], None, None)
