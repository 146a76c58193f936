"""`ops.matmul_integer_decode` / `ops.qlinear_matmul_decode` / `oq_qlinear_matmul_decode` (include/oq_hip_qlinear_decode.h,
csrc/qlinear_decode.hip): the decode route of QLinearMatMul, QGemm and MatMulInteger, M = 1 ... 16.  Every sum is an exact int32 and
the epilogue is the tile kernel's own code, so every check is an equality.

1  exact integers (OQ_QL_OUT_I32): `torch.equal` with the int64 product made on the CPU -- every row tier, sign combination, layout
   and zero-point form over a table of (K, N) at the edges of the plan's units, strides and odd bases, a bias, large grids.
2  epilogues: the bytes of the NumPy restatement and of `oq_qlinear_matmul` on the same operands.
3  refusals, and no expanded operand in memory.
"""
import numpy as np
import pytest
import torch

from qlinear_cases import DT, KN, LAYOUTS, NK, OUT_F32, OUT_I8, OUT_I32, OUT_U8, RANGE, SIGNS, Case, gen, raw, restate
from qlinear_decode_cases import plan, raw_decode, workspace

pytestmark = pytest.mark.gpu

ROWS = [1, 2, 4, 5, 8, 9, 16]                      # both ends of every tier
ZPS = ["lo", "hi", "mid", "null", "a_null", "b_null"]


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


def describe(wrong, c):
    idx = wrong.nonzero()
    return (f"{int(wrong.sum())} of {wrong.numel()} wrong, rows {sorted(set(idx[:, 0].tolist()))[:8]}, columns {sorted(set(idx[:, 1].tolist()))[:12]} "
            f"(plan {plan(c.M, c.K, c.N, c.layout)})")


# ------------------------------------------------------------------------------------ 1. exact integers
# (K, N): K one short of / at / one past a dot4 (4), a 16-byte load and a KN stage (16), the KN slice unit (64), the NK slice and wave
# span (1024), and slices with a short last one (1025, 2050; in KN also 65, 255 ...); N at 1, 3 / 4 / 5 (a KN lane's four columns),
# 15 / 16 / 17 (an NK iteration and column unit), 255 / 256 / 257 (a KN workgroup's columns).
TABLE = [(1, 1), (3, 5), (4, 4), (5, 3), (15, 16), (16, 63), (17, 64), (63, 65), (64, 255), (65, 17), (1023, 15), (1024, 256), (1025, 257), (2050, 70)]


def test_the_table_sits_on_the_edges_of_the_plan():
    assert plan(1, 1024, 256, NK).splits == 1 and plan(1, 1025, 257, NK).splits == 2 and plan(16, 2050, 70, NK)[1:3] + (plan(16, 2050, 70, NK).last,) == (1024, 3, 2)
    assert plan(1, 1024, 256, NK).cols_per_block == 16 and plan(1, 1024, 256, NK).col_blocks == 16 and plan(1, 17, 64, NK).col_blocks == 4
    assert plan(9, 1025, 257, NK).col_blocks == 17                                  # the last workgroup has one row of B
    assert plan(1, 64, 255, KN).splits == 1 and plan(1, 65, 17, KN)[1:3] == (64, 2) and plan(1, 65, 17, KN).last == 1
    assert plan(1, 1024, 256, KN)[1:3] == (64, 16) and plan(16, 1024, 256, KN)[1:3] == (64, 16)
    assert plan(1, 1025, 257, KN).col_blocks == 2 and plan(1, 1025, 257, KN)[1:3] == (64, 17)
    assert plan(16, 2050, 70, KN)[1:3] == (64, 33) and plan(16, 2050, 70, KN).last == 2
    # a KN slice of several stages per wave: at these widths only
    assert plan(16, 11008, 4096, KN).slice == 704 and plan(1, 4096, 11008, KN).slice == 384


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("signs", SIGNS, ids=sign_id)
def test_exact_integers_over_the_plan_sweep(ops, signs, layout):
    """Every (K, N) of the table at every M; the zero-point form walks along, so that each form meets each M and each table row.
    The full product of forms and rows follows below on two table rows."""
    bad = []
    for i, (K, N) in enumerate(TABLE):
        for j, M in enumerate(ROWS):
            zp = ZPS[(i + j) % len(ZPS)]
            c = Case(gen(1000 + 10 * i + j), M, K, N, signs[0], signs[1], LAYOUTS[layout], zp=zp)
            got = c_matmul_integer_decode(ops, c)
            assert got.dtype == torch.int32 and got.shape == (M, N)
            wrong = got.cpu() != c.want_i32()
            if wrong.any():
                bad.append(f"{(M, K, N, zp)}: {describe(wrong, c)}")
    assert not bad, "\n".join(bad)


def c_matmul_integer_decode(ops, c, a=None, b=None):
    return ops.matmul_integer_decode(c.a if a is None else a, c.b if b is None else b, c.a_zp, c.b_zp, trans_b=c.trans_b)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("signs", SIGNS, ids=sign_id)
def test_exact_integers_for_every_zero_point_form_at_every_row_count(ops, lib, signs, layout):
    """(K, N) = (65, 17): one slice in NK, two in KN with a last slice of one k; (2050, 70): three / 33 slices.  Odd rows carry a bias
    near +-2^20 (through the entry point: MatMulInteger has none)."""
    bad = []
    for K, N in ((65, 17), (2050, 70)):
        for M in ROWS:
            for zp in ZPS:
                c = Case(gen(2000 + M), M, K, N, signs[0], signs[1], LAYOUTS[layout], zp=zp, bias=M % 2 == 1)
                if c.bias is not None:
                    assert int(c.bias.max()) > 1 << 20 and int(c.bias.min()) < -(1 << 20)
                st, got = raw_decode(lib, c)
                assert st == 0
                wrong = got.cpu() != c.want_i32()
                if wrong.any():
                    bad.append(f"{(M, K, N, zp)}: {describe(wrong, c)}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_the_pad_is_applied_after_the_flip(ops, layout):
    """An unsigned operand with a zero point of 0: a padded k or row must be a zero of the FLIPPED operand (a pad applied before the flip
    would be -128 there), in the product and in both sums."""
    for signs in (("u8", "i8"), ("i8", "u8"), ("u8", "u8")):
        for M, K, N in ((3, 65, 17), (9, 1025, 33)):
            c = Case(gen(13), M, K, N, signs[0], signs[1], LAYOUTS[layout], zp="null")
            c.a_zp = torch.zeros((), dtype=c.a.dtype, device="cuda")
            c.b_zp = torch.zeros((), dtype=c.b.dtype, device="cuda")
            wrong = c_matmul_integer_decode(ops, c).cpu() != c.want_i32()
            assert not wrong.any(), describe(wrong, c)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("signs", SIGNS, ids=sign_id)
def test_views_with_gaps_and_odd_bases_give_the_contiguous_bytes(lib, signs, layout):
    """lda > K, ldb with a gap, ldy > N with the gap columns keeping their sentinel, A and B at odd byte offsets with odd leading
    dimensions (KN rows 1-byte aligned, NK rows and A's rows not 16-byte aligned), N = 130 in KN with ldb = 130 (rows 2-byte aligned);
    the bytes beyond K and N are 77s, not zeros."""
    for M, K, N in ((1, 200, 130), (3, 1088, 100), (16, 65, 260), (9, 1088, 40)):
        c = Case(gen(11), M, K, N, signs[0], signs[1], LAYOUTS[layout], zp="lo")
        st, aligned = raw_decode(lib, c)
        assert st == 0 and torch.equal(aligned.cpu(), c.want_i32())
        rows_b, cols_b = c.b.shape
        assert c.layout == NK or N != 130 or (c.b.stride(0) == 130 and c.b.data_ptr() % 4 == 0)          # the 2-byte aligned rows
        # gaps
        wa = torch.full((M, K + 24), 77, dtype=c.a.dtype, device="cuda")
        wa[:, :K] = c.a
        wb = torch.full((rows_b, cols_b + 20), 77, dtype=c.b.dtype, device="cuda")
        wb[:, :cols_b] = c.b
        y = torch.full((M, N + 5), -77, dtype=torch.int32, device="cuda")
        st, _ = raw_decode(lib, c, a=wa[:, :K], lda=K + 24, b=wb[:, :cols_b], ldb=cols_b + 20, y=y, ldy=N + 5)
        assert st == 0 and torch.equal(y[:, :N], aligned) and (y[:, N:] == -77).all()
        # odd bases and odd leading dimensions
        oa = torch.full((M * (K + 3) + 1,), 77, dtype=c.a.dtype, device="cuda")
        va = oa[1:].reshape(M, K + 3)[:, :K]
        va.copy_(c.a)
        ob = torch.full((rows_b * (cols_b + 3) + 3,), 77, dtype=c.b.dtype, device="cuda")
        vb = ob[3:].reshape(rows_b, cols_b + 3)[:, :cols_b]
        vb.copy_(c.b)
        assert va.data_ptr() % 2 == 1 and vb.data_ptr() % 2 == 1
        st, got = raw_decode(lib, c, a=va, lda=K + 3, b=vb, ldb=cols_b + 3)
        assert st == 0 and torch.equal(got, aligned)
        # one operand odd at a time: each load path on its own
        st, got = raw_decode(lib, c, a=va, lda=K + 3)
        assert st == 0 and torch.equal(got, aligned)
        st, got = raw_decode(lib, c, b=vb, ldb=cols_b + 3)
        assert st == 0 and torch.equal(got, aligned)
        # 2-byte aligned rows of B (an even base, ldb = 2 mod 4)
        ld2 = cols_b + 1 + (1 - cols_b) % 4                                  # the first leading dimension past cols_b that is 2 mod 4
        ob2 = torch.full((rows_b * ld2 + 2,), 77, dtype=c.b.dtype, device="cuda")
        vb2 = ob2[2:].reshape(rows_b, ld2)[:, :cols_b]
        vb2.copy_(c.b)
        assert ld2 % 4 == 2 and ld2 > cols_b and vb2.data_ptr() % 4 == 2
        st, got = raw_decode(lib, c, b=vb2, ldb=ld2)
        assert st == 0 and torch.equal(got, aligned)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_slices_of_several_stages_and_many_slabs(ops, layout):
    """K = 32900: 33 slices in NK.  In KN the slice grows past its unit only when K is long against the columns: 320 k at M = 16 (five
    stages a wave, and A's slice staged in two rounds), 128 k at M = 1."""
    for M, K, N, kn_slice in ((16, 32900, 300, 320), (1, 32900, 3, 128)):
        assert plan(M, K, N, KN).slice == kn_slice and plan(M, K, N, NK).splits == 33
        c = Case(gen(83), M, K, N, "u8", "i8", LAYOUTS[layout], zp="lo")
        wrong = c_matmul_integer_decode(ops, c).cpu() != c.want_i32()
        assert not wrong.any(), describe(wrong, c)


@pytest.mark.parametrize("signs", SIGNS, ids=sign_id)
def test_both_routes_of_the_upper_tiers_of_an_nk_matrix(lib, signs):
    """M = 5 ... 16 against a B stored [N, K] runs on the matrix cores where the rows of B are 16-byte aligned and K is a multiple of
    16, and on dot4 otherwise.  K = 48 (one span, three of its four 16-byte chunks), 1040 (a second slice of 16 k), 2064 (three slices);
    N with partial tiles; every zero-point form.  The same operands in a buffer whose rows are 8-byte aligned take the dot4 route and
    must give the same bytes."""
    bad = []
    for i, (K, N) in enumerate(((48, 17), (1040, 33), (2064, 70))):
        for j, M in enumerate((5, 8, 9, 16)):
            for zp in (ZPS[(i + j) % 6], ZPS[(i + j + 3) % 6]):
                c = Case(gen(3000 + 10 * i + j), M, K, N, signs[0], signs[1], NK, zp=zp, bias=(i + j) % 2 == 0)
                assert c.b.data_ptr() % 16 == 0 and c.b.stride(0) % 16 == 0
                st, got = raw_decode(lib, c)
                assert st == 0
                wrong = got.cpu() != c.want_i32()
                if wrong.any():
                    bad.append(f"{(M, K, N, zp)} on the matrix cores: {describe(wrong, c)}")
                wide = torch.full((N, K + 8), 77, dtype=c.b.dtype, device="cuda")
                wide[:, :K] = c.b
                st, other = raw_decode(lib, c, b=wide[:, :K], ldb=K + 8)
                assert st == 0
                if not torch.equal(other, got):
                    bad.append(f"{(M, K, N, zp)}: the dot4 route differs from the matrix cores")
    assert not bad, "\n".join(bad)


def smallest_large_grid(M, layout):
    """The smallest (K, N) whose plan has at least 512 workgroups in one slice: more than two per compute unit."""
    if layout == NK:
        K, N = 64, 512 * 16
    else:
        K, N = 64, 512 * 256
    pl = plan(M, K, N, layout)
    assert pl.grid == 512 and pl.splits == 1
    assert plan(M, K, N - pl.cols_per_block, layout).grid < 512
    return K, N


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("M", [1, 16])
def test_exact_integers_on_a_grid_of_several_workgroups_per_cu(ops, lib, M, layout):
    """512 workgroups: more than the 256 CUs, so waves of different workgroups share a SIMD (the lesson of docs/LAB_NOTES_r22.md,
    section 2).  Four calls, each exact, and the four results bytewise equal.  Next to it a grid of 512 workgroups made of slices
    (slabs and the second launch)."""
    K, N = smallest_large_grid(M, LAYOUTS[layout])
    for K, N in ((K, N), (4096 if layout == "NK" else 2048, 2048 if layout == "NK" else 4096)):
        c = Case(gen(19), M, K, N, "u8", "i8", LAYOUTS[layout], zp="lo")
        pl = plan(M, K, N, c.layout)
        assert pl.grid >= 256 and lib.oq_qlinear_matmul_decode_workspace_bytes(M, K, N, c.layout) == workspace(M, K, N, c.layout)
        want = c.want_i32().cuda()
        got = [c_matmul_integer_decode(ops, c) for _ in range(4)]
        wrong = [g != want for g in got]
        for i, w in enumerate(wrong):
            if w.any():
                print(f"call {i}: {describe(w.cpu(), c)}")
        assert [int(w.sum()) for w in wrong] == [0, 0, 0, 0]
        assert all(torch.equal(g, got[0]) for g in got[1:])


# ------------------------------------------------------------------------------------ 2. epilogues
def scalar(v, dtype=torch.float32):
    return torch.tensor(v, dtype=dtype, device="cuda")


EPILOGUES = [(out, per_column) for out in (OUT_F32, OUT_U8, OUT_I8) for per_column in (False, True)]


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("out,per_column", EPILOGUES, ids=[f"{['i32', 'f32', 'u8', 'i8'][o]}-{'column' if p else 'tensor'}" for o, p in EPILOGUES])
def test_epilogues_have_the_bytes_of_the_restatement_and_of_the_tile_kernel(lib, out, per_column, layout):
    """Span-limited operands (accumulators that fill the output type without living at its ends), random scales with full
    significands; finished by the first launch (one slice) and by the second (slabs)."""
    shapes = (((16, 64, 130), ("u8", "i8")), ((3, 1088, 100), ("i8", "u8"))) if layout == "NK" else (((16, 64, 300), ("u8", "i8")), ((3, 1088, 100), ("i8", "u8")))
    for (M, K, N), signs in shapes:
        c = Case(gen(23), M, K, N, signs[0], signs[1], LAYOUTS[layout], zp="mid", bias=True, span=20)
        assert (plan(M, K, N, c.layout).splits == 1) == (K == 64)
        if per_column:                                                      # the C ABI takes one flag for b_scale and b_zero_point
            c.b_zp = c.b_zp.reshape(1).expand(N).contiguous()
        g = gen(29)
        a_s = scalar(0.0123456789)
        b_s = (torch.rand((N,), device="cuda", generator=g) * 0.02 + 0.001) if per_column else scalar(0.00987654321)
        acc = c.acc.numpy()
        s64 = float(a_s) * b_s.double().cpu().numpy().reshape(1, -1)
        kw = dict(out=out, a_scale=a_s, b_scale=b_s)
        if out == OUT_F32:
            want = restate(acc, a_s.item(), b_s.cpu().numpy())
            view = np.uint32
        else:
            dtype = torch.uint8 if out == OUT_U8 else torch.int8
            lo, hi = RANGE[dtype]
            y_s = scalar(float(np.abs(acc * s64).max()) / 100.0)
            y_zp = torch.tensor((lo + hi + 1) // 2 + 3, dtype=dtype, device="cuda")
            kw.update(y_scale=y_s, y_zp=y_zp)
            want = restate(acc, a_s.item(), b_s.cpu().numpy(), y_s.item(), int(y_zp), dtype)
            view = want.dtype
            assert len(np.unique(want)) > 40                                # the outputs do spread over the range
        st, got = raw_decode(lib, c, **kw)
        st_tile, tile = raw(lib, c, **kw)
        assert st == 0 and st_tile == 0
        assert np.array_equal(got.cpu().numpy().view(view), want.view(view))
        assert torch.equal(got.view(torch.uint8), tile.view(torch.uint8))


@pytest.mark.parametrize("dt", ["u8", "i8"])
def test_ties_round_half_to_even(ops, dt):
    """Scales 2^-3 and 2^-4 against y_scale 2^-6: t / y_scale = acc / 2 exactly, a tie wherever acc is odd."""
    dtype = DT[dt]
    lo, hi = RANGE[dtype]
    for layout in (KN, NK):
        c = Case(gen(37), 16, 64, 130, "u8", "i8", layout, zp="mid", span=3)
        acc = c.acc.numpy()
        y_zp = torch.tensor((lo + hi + 1) // 2, dtype=dtype, device="cuda")
        args = (c.a, scalar(0.125), c.a_zp, c.b, scalar(0.0625), c.b_zp, scalar(0.015625), y_zp)
        got = ops.qlinear_matmul_decode(*args, trans_b=c.trans_b)
        assert torch.equal(got, ops.qlinear_matmul(*args, trans_b=c.trans_b))
        got = got.cpu().numpy().astype(np.int64)
        ties = acc % 2 != 0
        assert ties.mean() >= 0.25 and ((acc / 2 + int(y_zp) > lo + 1) & (acc / 2 + int(y_zp) < hi - 1)).all()
        assert np.array_equal(got, restate(acc, 0.125, 0.0625, 0.015625, int(y_zp), dtype).astype(np.int64))
        level = got - int(y_zp)
        assert (level[ties] % 2 == 0).all() and (np.abs(level[ties] - acc[ties] / 2) == 0.5).all()


@pytest.mark.parametrize("dt", ["u8", "i8"])
def test_saturation_at_both_ends(ops, dt):
    dtype = DT[dt]
    lo, hi = RANGE[dtype]
    for layout in (KN, NK):
        c = Case(gen(41), 9, 200, 130, "u8", "i8", layout, zp="mid")
        a_s, b_s, y_s = scalar(0.05), scalar(0.03), scalar(0.1)
        y_zp = torch.tensor((lo + hi + 1) // 2, dtype=dtype, device="cuda")
        got = ops.qlinear_matmul_decode(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s, y_zp, trans_b=c.trans_b)
        assert torch.equal(got, ops.qlinear_matmul(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s, y_zp, trans_b=c.trans_b))
        got = got.cpu().numpy()
        assert np.array_equal(got, restate(c.acc.numpy(), a_s.item(), b_s.item(), y_s.item(), int(y_zp), dtype))
        r = c.acc.numpy() * (0.05 * 0.03 / 0.1) + int(y_zp)
        assert (r > hi + 10).any() and (r < lo - 10).any()
        assert (got[r > hi + 10] == hi).all() and (got[r < lo - 10] == lo).all()


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_every_output_code_on_an_extreme_case_equals_the_tile_route(ops, layout):
    """Operands over the whole range of their types, extremes forced, per-column parameters, a bias: int32, fp32, uint8 and int8."""
    M, K, N = 16, 1030, 260
    c = Case(gen(43), M, K, N, "u8", "i8", LAYOUTS[layout], zp="lo", bias=True)
    assert torch.equal(c_matmul_integer_decode(ops, c), c.matmul_integer(ops))
    a_s = scalar(0.02)
    b_s = torch.rand((N,), device="cuda", generator=gen(47)) * 0.004 + 0.008
    y_s = scalar(float(c.acc.abs().max()) * 0.02 * 0.012 / 100.0)
    common = dict(bias=c.bias, trans_b=c.trans_b)
    got = ops.qlinear_matmul_decode(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, **common)
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), ops.qlinear_matmul(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, **common).view(torch.int32))
    for y_zp in (None, torch.tensor(131, dtype=torch.uint8, device="cuda"), torch.tensor(-5, dtype=torch.int8, device="cuda")):
        got = ops.qlinear_matmul_decode(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s, y_zp, **common)
        assert got.dtype == (torch.uint8 if y_zp is None else y_zp.dtype) and got.shape == (M, N)
        assert torch.equal(got, ops.qlinear_matmul(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s, y_zp, **common))
        assert len(torch.unique(got)) > 40


# ------------------------------------------------------------------------------------ 3. refusals, memory
def test_refusals_leave_y_untouched_and_the_op_raises_by_name(ops, lib):
    c = Case(gen(61), 8, 64, 16, "u8", "i8", KN, zp="mid")
    a_s, b_s, y_s = scalar(0.02), scalar(0.01), scalar(0.5)
    y = torch.full((17, 16), 99, dtype=torch.uint8, device="cuda")
    a17 = torch.zeros((17, 64), dtype=torch.uint8, device="cuda")
    for kw, status, word in ((dict(flags=1), -2, "per-row"), (dict(flags=2), -2, "transA"), (dict(flags=4), -2, "alpha"),
                             (dict(a=a17, M=17), -2, "M = 17 rows"), (dict(a_code=5), -1, "a_type"), (dict(b_code=5), -1, "b_type"),
                             (dict(layout=7), -1, "b_layout"), (dict(out_code=9), -1, "out"), (dict(ldy=15), -1, "ldy=15")):
        st, _ = raw_decode(lib, c, out=OUT_U8, a_scale=a_s, b_scale=b_s, y_scale=y_s, y=y, **{"ldy": 16, **kw})
        assert st == status, (kw, st)
        assert word in lib.oq_last_error().decode()
    assert (y == 99).all()
    st, _ = raw_decode(lib, c, out=OUT_U8, a_scale=a_s, b_scale=b_s, y_scale=y_s, y=y[:8], ldy=16)
    assert st == 0 and np.array_equal(y[:8].cpu().numpy(), restate(c.acc.numpy(), 0.02, 0.01, 0.5, 0, torch.uint8)) and (y[8:] == 99).all()

    with pytest.raises(NotImplementedError, match="17 rows"):
        ops.qlinear_matmul_decode(a17, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s)
    with pytest.raises(NotImplementedError, match="17 rows"):
        ops.matmul_integer_decode(a17.reshape(17, 1, 64), c.b, c.a_zp, c.b_zp)
    with pytest.raises(NotImplementedError, match="per-row a_scale"):
        ops.qlinear_matmul_decode(c.a, torch.full((8,), 0.02, device="cuda"), c.a_zp, c.b, b_s, c.b_zp, y_s)
    with pytest.raises(NotImplementedError, match="not fp32"):
        ops.qlinear_matmul_decode(c.a, a_s.half(), c.a_zp, c.b, b_s, c.b_zp, y_s)
    with pytest.raises(NotImplementedError, match="alpha"):
        ops.qlinear_matmul_decode(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s, alpha=0.5)
    with pytest.raises(NotImplementedError, match="transA"):
        ops.qlinear_matmul_decode(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s, trans_a=True)
    assert ops.qlinear_matmul_decode_unsupported(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s) is None
    assert "17 rows" in ops.qlinear_matmul_decode_unsupported(a17, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s)
    assert "40 rows" in ops.qlinear_matmul_decode_unsupported(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s, rows=40)
    assert ops.qlinear_matmul_unsupported(a17, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s) is None      # the tile route's refusals are what they were


def test_leading_axes_are_flattened_and_restored_and_an_empty_input_returns_empty(ops):
    c = Case(gen(71), 12, 96, 40, "u8", "i8", NK, zp="lo")
    y = ops.matmul_integer_decode(c.a.reshape(2, 3, 2, 96), c.b, c.a_zp, c.b_zp, trans_b=True)
    assert y.shape == (2, 3, 2, 40) and torch.equal(y.reshape(12, 40).cpu(), c.want_i32())
    empty = ops.matmul_integer_decode(c.a[:0].reshape(0, 3, 96), c.b, c.a_zp, c.b_zp, trans_b=True)
    assert empty.shape == (0, 3, 40) and empty.dtype == torch.int32


def test_no_expanded_operand_is_ever_allocated(ops, lib):
    """Peak memory of a call at 16 x 1024 x 1024 stays within the output plus the workspace (the allocator rounds each to 512 B)."""
    M, K, N = 16, 1024, 1024
    for layout in (KN, NK):
        c = Case(gen(51), M, K, N, "u8", "i8", layout, zp="mid")
        a_s, b_s, y_s, y_zp = scalar(0.02), scalar(0.01), scalar(4.0), torch.tensor(128, dtype=torch.uint8, device="cuda")
        call = lambda: ops.qlinear_matmul_decode(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s, y_zp, trans_b=c.trans_b)      # noqa: E731
        call()                                                              # the library is loaded
        torch.cuda.synchronize()
        torch.cuda.empty_cache()      # no cached block of another size is handed out whole: the figures are the requests, rounded to 512 B
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = call()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        need = workspace(M, K, N, layout)
        allowed = -(-M * N // 512) * 512 + (-(-need // 512) * 512 if need else 0)
        print(f"layout {layout}: peak growth {peak} B, output {M * N} B, workspace {need} B, a dequantized weight {K * N * 4} B")
        assert peak <= allowed < K * N * 4
        del out
