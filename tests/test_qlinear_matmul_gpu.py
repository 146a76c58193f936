"""`ops.matmul_integer` / `ops.qlinear_matmul` / `oq_qlinear_matmul` (include/oq_hip_qlinear.h, csrc/qlinear_gemm.hip): QLinearMatMul,
QGemm and MatMulInteger on the int8 matrix cores.

1  exact integers (OQ_QL_OUT_I32): `torch.equal` with the int64 product made on the CPU -- a table of shapes, every sign combination,
   both layouts of B, zero points at the ends of their types, strides and odd bases, a bias, grids of several workgroups per CU.
2  epilogues: bit equality with the NumPy restatement of the stated order, ties, saturation, and a float64 bound.
3  routes: beside the expansion of `GraphRunner._op_QLinearMatMul`, no dequantized weight in memory, refusals.
"""
import numpy as np
import pytest
import torch

from nbits_cases import describe
from qlinear_cases import (DT, KN, LAYOUTS, NK, OUT_F32, OUT_I8, OUT_I32, OUT_U8, RANGE, SIGNS, Case, gen, raw, restate, workspace)

pytestmark = pytest.mark.gpu


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


# ------------------------------------------------------------------------------------ 1. exact integers
# (M, K, N, zero points (qlinear_cases.Case), what the row is there for).  K * 255^2 < 2^31 throughout.
SWEEP = [
    (1, 1, 1, "lo", "one output, K below one step, one extreme pair only"),
    (16, 63, 100, "lo", "K one short of a step; a partial column tile"),
    (16, 64, 130, "hi", "exactly one step; a second column tile of two columns"),
    (16, 65, 1, "b_null", "K one past a step: a second step of one k; one column"),
    (33, 65, 100, "lo", "the 128-row tile, partial; K one past a step (the pad comes after the flip)"),
    (33, 200, 260, "null", "no zero points: no sums for signed operands; three column tiles, the last of four columns"),
    (129, 200, 260, "lo", "two row tiles, the second of one row; 6 tiles x 4 steps: one step a block"),
    (129, 64, 1, "hi", "one column under two row tiles"),
    (1, 200, 100, "a_null", "one row; several steps in four blocks along K"),
    (1, 1088, 1, "lo", "split K, 17 steps as 3 + 3 + 3 + 3 + 3 + 2: a short last split (32-row tile)"),
    (16, 1088, 260, "mid", "split K with a short last split on three column tiles"),
    (33, 1088, 130, "lo", "split K with a short last split on the 128-row tile"),
    (129, 1088, 100, "hi", "split K on two row tiles"),
    (129, 1088, 130, "a_null", "split K, four tiles, several steps per block: 17 steps as 3 + ... + 2"),
]


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("signs", SIGNS, ids=sign_id)
def test_exact_integers_over_the_table(ops, signs, layout):
    bad = []
    for i, (M, K, N, zp, why) in enumerate(SWEEP):
        c = Case(gen(100 + i), M, K, N, signs[0], signs[1], LAYOUTS[layout], zp=zp)
        got = c.matmul_integer(ops)
        assert got.dtype == torch.int32 and got.shape == (M, N)
        wrong = got.cpu() != c.want_i32()
        if wrong.any():
            bad.append(f"{(M, K, N, zp)} [{why}]: {describe(wrong, c.plan())}")
    assert not bad, "\n".join(bad)


def test_the_table_covers_what_it_names():
    """The plans behind the rows: a short last split, several steps per block, both tile heights."""
    from nbits_cases import plan
    pl = plan(16, 1088, 260)
    assert (pl.bm, pl.tiles, pl.steps, pl.steps_per_split, pl.splits, pl.last) == (32, 3, 17, 3, 6, 2)
    pl = plan(33, 1088, 130)
    assert (pl.bm, pl.tiles, pl.steps_per_split, pl.splits, pl.last) == (128, 2, 3, 6, 2)
    assert plan(129, 200, 260).splits == 4 and plan(1, 200, 100).splits == 4 and plan(33, 65, 100).splits == 2
    assert {m for m, *_ in SWEEP} == {1, 16, 33, 129} and {k for _, k, *_ in SWEEP} == {1, 63, 64, 65, 200, 1088}
    assert {n for _, _, n, *_ in SWEEP} == {1, 100, 130, 260}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("signs", SIGNS, ids=sign_id)
def test_several_steps_in_one_block_with_a_partial_last_step(ops, signs, layout):
    """K stays in one block (no slabs; the GEMM kernel itself corrects and finishes) only from 128 tiles on: 129 tiles of the 32-row
    kernel, the last of 16 columns, K = 200 as 64 + 64 + 64 + 8."""
    c = Case(gen(7), 16, 200, 16400, signs[0], signs[1], LAYOUTS[layout], zp="lo")
    assert c.plan().splits == 1 and c.plan().tiles == 129 and c.plan().steps == 4
    wrong = c.matmul_integer(ops).cpu() != c.want_i32()
    assert not wrong.any(), describe(wrong, c.plan())


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("signs", SIGNS, ids=sign_id)
def test_views_with_gaps_and_odd_bases_give_the_aligned_bytes(lib, signs, layout):
    """lda > K, ldb > N (KN) / ldb > K (NK), ldy > N with the gap columns keeping their sentinel, bases at odd byte offsets (narrower
    loads), and N = 130 in KN with ldb = 130: rows of B that are 2-byte aligned."""
    for M, K, N in ((33, 200, 130), (3, 1088, 100), (16, 65, 260)):
        c = Case(gen(11), M, K, N, signs[0], signs[1], LAYOUTS[layout], zp="lo")
        st, aligned = raw(lib, c)
        assert st == 0 and torch.equal(aligned.cpu(), c.want_i32())
        rows_b, cols_b = c.b.shape
        assert c.layout == NK or N != 130 or (c.b.stride(0) == 130 and c.b.data_ptr() % 4 == 0)          # the 2-byte aligned rows
        # gaps
        wa = torch.full((M, K + 24), 77, dtype=c.a.dtype, device="cuda")
        wa[:, :K] = c.a
        wb = torch.full((rows_b, cols_b + 20), 77, dtype=c.b.dtype, device="cuda")
        wb[:, :cols_b] = c.b
        y = torch.full((M, N + 5), -77, dtype=torch.int32, device="cuda")
        st, _ = raw(lib, c, a=wa[:, :K], b=wb[:, :cols_b], y=y, ldy=N + 5)
        assert st == 0 and torch.equal(y[:, :N], aligned) and (y[:, N:] == -77).all()
        # odd bases and odd leading dimensions
        oa = torch.full((M * (K + 3) + 1,), 77, dtype=c.a.dtype, device="cuda")
        va = oa[1:].reshape(M, K + 3)[:, :K]
        va.copy_(c.a)
        ob = torch.full((rows_b * (cols_b + 3) + 3,), 77, dtype=c.b.dtype, device="cuda")
        vb = ob[3:].reshape(rows_b, cols_b + 3)[:, :cols_b]
        vb.copy_(c.b)
        assert va.data_ptr() % 2 == 1 and vb.data_ptr() % 2 == 1
        st, got = raw(lib, c, a=va, lda=K + 3, b=vb, ldb=cols_b + 3)
        assert st == 0 and torch.equal(got, aligned)
        # one operand odd at a time: each staging path on its own
        st, got = raw(lib, c, a=va, lda=K + 3)
        assert st == 0 and torch.equal(got, aligned)
        st, got = raw(lib, c, b=vb, ldb=cols_b + 3)
        assert st == 0 and torch.equal(got, aligned)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_the_pad_is_applied_after_the_flip(ops, layout):
    """K = 65 with an unsigned A and a_zp = 0 (and the same for B): the 63 padded k of the second step must be zeros of the FLIPPED
    operand.  A pad applied before the flip would be -128 there."""
    for signs in (("u8", "i8"), ("i8", "u8"), ("u8", "u8")):
        c = Case(gen(13), 33, 65, 100, signs[0], signs[1], LAYOUTS[layout], zp="null")
        c.a_zp = torch.zeros((), dtype=c.a.dtype, device="cuda")
        c.b_zp = torch.zeros((), dtype=c.b.dtype, device="cuda")
        wrong = c.matmul_integer(ops).cpu() != c.want_i32()
        assert not wrong.any(), describe(wrong, c.plan())


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_a_bias_is_added_to_the_accumulator(lib, layout):
    for M, K, N in ((33, 64, 130), (3, 1088, 100)):                        # finished by the GEMM kernel, and by the reduce kernel
        c = Case(gen(17), M, K, N, "u8", "i8", LAYOUTS[layout], zp="lo", bias=True)
        assert int(c.bias.max()) > 1 << 20 and int(c.bias.min()) < -(1 << 20)
        st, got = raw(lib, c)
        assert st == 0 and torch.equal(got.cpu(), c.want_i32())


LARGE_GRIDS = [(2048, 256, 4096), (16, 64, 65536)]


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("shape", LARGE_GRIDS, ids=str)
def test_exact_integers_on_grids_of_several_workgroups_per_cu(ops, lib, shape, layout):
    """512 tiles of each tile height, K in one pass: more workgroups than the 256 CUs, so waves of different workgroups share a SIMD
    (the lesson of docs/LAB_NOTES_r22.md, section 2).  Four calls, each exact, and the four results bytewise equal."""
    M, K, N = shape
    c = Case(gen(19), M, K, N, "u8", "i8", LAYOUTS[layout], zp="lo")
    pl = c.plan()
    assert pl.tiles == 512 and pl.splits == 1 and pl.bm == (128 if M > 32 else 32)
    assert lib.oq_qlinear_matmul_workspace_bytes(M, K, N) == workspace(M, K, N)
    want = c.want_i32().cuda()
    got = [c.matmul_integer(ops) for _ in range(4)]
    wrong = [g != want for g in got]
    for i, w in enumerate(wrong):
        if w.any():
            print(f"call {i}: {describe(w, pl)}")
    assert [int(w.sum()) for w in wrong] == [0, 0, 0, 0]
    assert all(torch.equal(g, got[0]) for g in got[1:])


# ------------------------------------------------------------------------------------ 2. epilogues
def scalar(v, dtype=torch.float32):
    return torch.tensor(v, dtype=dtype, device="cuda")


EPILOGUES = [(out, per_column) for out in (OUT_F32, OUT_U8, OUT_I8) for per_column in (False, True)]


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("out,per_column", EPILOGUES, ids=[f"{['i32', 'f32', 'u8', 'i8'][o]}-{'column' if p else 'tensor'}" for o, p in EPILOGUES])
def test_epilogues_equal_the_numpy_restatement_bit_for_bit(ops, out, per_column, layout):
    """Random scales with full significands; y_scale sized so that the outputs fill the type's range without living at its ends.
    Also against float64: three fp32 roundings (conversion, product, quotient) lie between the exact value and the rounded one."""
    for (M, K, N), signs in (((33, 64, 130), ("u8", "i8")), ((3, 1088, 100), ("i8", "u8"))):      # finished by the GEMM / the reduce kernel
        c = Case(gen(23), M, K, N, signs[0], signs[1], LAYOUTS[layout], zp="mid", bias=True)
        g = gen(29)
        a_s = scalar(0.0123456789)
        b_s = (torch.rand((N,), device="cuda", generator=g) * 0.02 + 0.001) if per_column else scalar(0.00987654321)
        acc = c.acc.numpy()
        s64 = float(a_s) * b_s.double().cpu().numpy().reshape(1, -1)
        if out == OUT_F32:
            got = ops.qlinear_matmul(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, bias=c.bias, trans_b=c.trans_b)
            assert got.dtype == torch.float32
            want = restate(acc, a_s.item(), b_s.cpu().numpy())
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
            assert (np.abs(got.double().cpu().numpy() - acc * s64) <= 2 * 2.0 ** -24 * np.abs(acc * s64)).all()
            continue
        dtype = torch.uint8 if out == OUT_U8 else torch.int8
        lo, hi = RANGE[dtype]
        y_s = scalar(float(np.abs(acc * s64).max()) / 100.0)
        y_zp = torch.tensor((lo + hi + 1) // 2 + 3, dtype=dtype, device="cuda")
        got = ops.qlinear_matmul(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s, y_zp, bias=c.bias, trans_b=c.trans_b)
        assert got.dtype == dtype and got.shape == (M, N)
        want = restate(acc, a_s.item(), b_s.cpu().numpy(), y_s.item(), int(y_zp), dtype)
        assert np.array_equal(got.cpu().numpy(), want)
        r = acc * s64 / float(y_s)
        err = np.abs(got.cpu().numpy().astype(np.float64) - np.clip(r + int(y_zp), lo, hi))
        assert (err <= 0.5 + 3 * 2.0 ** -24 * np.abs(r)).all(), (err - 0.5 - 3 * 2.0 ** -24 * np.abs(r)).max()
        assert len(np.unique(want)) > 40                                    # the outputs do spread over the range


def test_a_missing_y_zero_point_gives_uint8_around_zero(ops):
    c = Case(gen(31), 16, 64, 100, "u8", "i8", KN, zp="mid")
    a_s, b_s, y_s = scalar(0.02), scalar(0.01), scalar(0.5)
    got = ops.qlinear_matmul(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s)
    assert got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), restate(c.acc.numpy(), a_s.item(), b_s.item(), y_s.item(), 0, torch.uint8))


@pytest.mark.parametrize("dt", ["u8", "i8"])
def test_ties_round_half_to_even(ops, dt):
    """Scales 2^-3 and 2^-4 against y_scale 2^-6: t / y_scale = acc / 2 exactly, a tie wherever acc is odd."""
    dtype = DT[dt]
    lo, hi = RANGE[dtype]
    c = Case(gen(37), 33, 64, 130, "u8", "i8", KN, zp="mid", span=3)
    acc = c.acc.numpy()
    y_zp = torch.tensor((lo + hi + 1) // 2, dtype=dtype, device="cuda")
    got = ops.qlinear_matmul(c.a, scalar(0.125), c.a_zp, c.b, scalar(0.0625), c.b_zp, scalar(0.015625), y_zp).cpu().numpy().astype(np.int64)
    ties = acc % 2 != 0
    inside = (acc / 2 + int(y_zp) > lo + 1) & (acc / 2 + int(y_zp) < hi - 1)
    assert ties.mean() >= 0.25 and inside.all()
    assert np.array_equal(got, restate(acc, 0.125, 0.0625, 0.015625, int(y_zp), dtype).astype(np.int64))
    level = got - int(y_zp)
    assert (level[ties] % 2 == 0).all() and (np.abs(level[ties] - acc[ties] / 2) == 0.5).all()
    assert (level[~ties] == acc[~ties] // 2).all()


@pytest.mark.parametrize("dt", ["u8", "i8"])
def test_saturation_at_both_ends(ops, dt):
    dtype = DT[dt]
    lo, hi = RANGE[dtype]
    c = Case(gen(41), 33, 200, 130, "u8", "i8", KN, zp="mid")
    a_s, b_s, y_s = scalar(0.05), scalar(0.03), scalar(0.1)
    y_zp = torch.tensor((lo + hi + 1) // 2, dtype=dtype, device="cuda")
    got = ops.qlinear_matmul(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s, y_zp).cpu().numpy()
    assert np.array_equal(got, restate(c.acc.numpy(), a_s.item(), b_s.item(), y_s.item(), int(y_zp), dtype))
    r = c.acc.numpy() * (0.05 * 0.03 / 0.1) + int(y_zp)
    assert (r > hi + 10).any() and (r < lo - 10).any()
    assert (got == lo).any() and (got == hi).any() and (got[r > hi + 10] == hi).all() and (got[r < lo - 10] == lo).all()


# ------------------------------------------------------------------------------------ 3. routes
def expansion(c, a_s, b_s, y_s, y_zp):
    """The route a holder of such a file has without the kernel: `GraphRunner._op_QLinearMatMul` itself."""
    from onnx_quantize_amd.graph_runner import GraphRunner
    runner = GraphRunner.evaluator(21)
    zero = lambda t, like: torch.zeros((), dtype=like.dtype, device="cuda") if t is None else t      # noqa: E731
    return GraphRunner._op_QLinearMatMul(runner, None, [c.a, a_s, zero(c.a_zp, c.a), c.b, b_s, zero(c.b_zp, c.b), y_s, y_zp], {}, None)


@pytest.mark.parametrize("per_column", [False, True], ids=["tensor", "column"])
@pytest.mark.parametrize("signs", SIGNS, ids=sign_id)
def test_beside_the_expansion_route_by_at_most_one_level(ops, signs, per_column):
    """Both routes lie within 0.5 + delta of the real value r = acc s / y_s + zp, so their integers differ by at most 1 wherever
    delta < 0.25.  The expansion's delta: K + 3 fp32 roundings (two dequantizations, the sum of K products, the quotient), each at
    most 2^-24 of |A_f| @ |B_f|, over y_s.  The fused route's own delta is 3 * 2^-24 |r| (the test above)."""
    M, K, N = 33, 256, 130
    c = Case(gen(43), M, K, N, signs[0], signs[1], KN, zp="lo" if per_column else "mid")
    g = gen(47)
    a_s = scalar(0.02)
    b_s = (torch.rand((N,), device="cuda", generator=g) * 0.004 + 0.008) if per_column else scalar(0.01)
    a_f = (c.a.double() - float(c.a_zp)) * float(a_s)
    b_f = (c.b.double() - c.b_zp.double().reshape(1, -1)) * b_s.double().reshape(1, -1)
    real = a_f @ b_f
    y_s = scalar(float(real.abs().max()) / 120.0)
    delta = (K + 3) * 2.0 ** -24 * (a_f.abs() @ b_f.abs()) / float(y_s)
    assert float(delta.max()) < 0.25, float(delta.max())
    y_zp = torch.tensor(128, dtype=torch.uint8, device="cuda")
    assert float((real / float(y_s)).abs().max()) + 1 < 127                 # inside the type's range: no clip hides a difference
    fused = ops.qlinear_matmul(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s, y_zp)
    plain = expansion(c, a_s, b_s, y_s, y_zp)
    assert fused.dtype == plain.dtype == torch.uint8
    apart = (fused.int() - plain.int()).abs()
    print(f"{sign_id(signs)} {'column' if per_column else 'tensor'}: max delta {float(delta.max()):.2e}, "
          f"{float((apart != 0).double().mean()):.3%} of the positions differ")
    assert int(apart.max()) <= 1
    for got in (fused, plain):
        assert float((got.double() - 128 - real / float(y_s)).abs().max()) <= 0.5 + 0.25


def test_no_dequantized_weight_is_ever_allocated(ops):
    M, K, N = 16, 1024, 1024
    c = Case(gen(51), M, K, N, "u8", "i8", KN, zp="mid")
    a_s, b_s, y_s, y_zp = scalar(0.02), scalar(0.01), scalar(4.0), torch.tensor(128, dtype=torch.uint8, device="cuda")

    def growth(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()      # no cached block of another size is handed out whole: the figures are the requests, rounded to 512 B
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        del out
        return peak

    fused_call = lambda: ops.qlinear_matmul(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s, y_zp)      # noqa: E731
    fused_call()                                                           # the library is loaded
    fused, expanded = growth(fused_call), growth(lambda: expansion(c, a_s, b_s, y_s, y_zp))
    print(f"peak growth fused {fused} B, expansion route {expanded} B, fp32 weight {K * N * 4} B")
    assert fused < K * N * 4
    assert expanded > K * N * 4                                            # the route it replaces does pay it: the test is not vacuous


def test_refusals_leave_y_untouched_and_the_op_raises_by_name(ops, lib):
    c = Case(gen(61), 8, 64, 16, "u8", "i8", KN, zp="mid")
    a_s, b_s, y_s = scalar(0.02), scalar(0.01), scalar(0.5)
    y = torch.full((8, 16), 99, dtype=torch.uint8, device="cuda")
    for kw, status, word in ((dict(flags=1), -2, "per-row"), (dict(flags=2), -2, "transA"), (dict(flags=4), -2, "alpha"),
                             (dict(a_code=5), -1, "a_type"), (dict(b_code=5), -1, "b_type"), (dict(layout=7), -1, "b_layout"),
                             (dict(out_code=9), -1, "out"), (dict(ldy=15), -1, "ldy=15")):
        st, _ = raw(lib, c, out=OUT_U8, a_scale=a_s, b_scale=b_s, y_scale=y_s, y=y, **{"ldy": 16, **kw})
        assert st == status, (kw, st)
        assert word in lib.oq_last_error().decode()
    assert (y == 99).all()
    st, _ = raw(lib, c, out=OUT_U8, a_scale=a_s, b_scale=b_s, y_scale=y_s, y=y, ldy=16)
    assert st == 0 and np.array_equal(y.cpu().numpy(), restate(c.acc.numpy(), 0.02, 0.01, 0.5, 0, torch.uint8))

    with pytest.raises(NotImplementedError, match="per-row a_scale"):
        ops.qlinear_matmul(c.a, torch.full((8,), 0.02, device="cuda"), c.a_zp, c.b, b_s, c.b_zp, y_s)
    with pytest.raises(NotImplementedError, match="not fp32"):
        ops.qlinear_matmul(c.a, a_s.half(), c.a_zp, c.b, b_s, c.b_zp, y_s)
    with pytest.raises(NotImplementedError, match="3-D b"):
        ops.qlinear_matmul(c.a, a_s, c.a_zp, c.b.reshape(1, 64, 16), b_s, c.b_zp, y_s)
    with pytest.raises(NotImplementedError, match="alpha"):
        ops.qlinear_matmul(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s, alpha=0.5)
    with pytest.raises(NotImplementedError, match="transA"):
        ops.qlinear_matmul(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s, trans_a=True)
    assert ops.qlinear_matmul_unsupported(c.a, a_s, c.a_zp, c.b, b_s, c.b_zp, y_s) is None
    assert "per-row" in ops.qlinear_matmul_unsupported(c.a, torch.full((8,), 0.02, device="cuda"), c.a_zp, c.b, b_s, c.b_zp, y_s)


def test_leading_axes_are_flattened_and_restored_and_an_empty_input_returns_empty(ops):
    c = Case(gen(71), 24, 96, 40, "u8", "i8", NK, zp="lo")
    y = ops.matmul_integer(c.a.reshape(2, 3, 4, 96), c.b, c.a_zp, c.b_zp, trans_b=True)
    assert y.shape == (2, 3, 4, 40) and torch.equal(y.reshape(24, 40).cpu(), c.want_i32())
    empty = ops.matmul_integer(c.a[:0].reshape(0, 3, 96), c.b, c.a_zp, c.b_zp, trans_b=True)
    assert empty.shape == (0, 3, 40) and empty.dtype == torch.int32
    q = ops.qlinear_matmul(c.a[:0], torch.tensor(0.5, device="cuda"), c.a_zp, c.b, torch.tensor(0.5, device="cuda"), c.b_zp,
                           torch.tensor(0.5, device="cuda"), trans_b=True)
    assert q.shape == (0, 40) and q.dtype == torch.uint8
