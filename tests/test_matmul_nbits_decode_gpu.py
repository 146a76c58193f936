"""`ops.matmul_nbits_decode` / `oq_matmul_nbits_decode` (include/oq_hip_nbits_decode.h, csrc/matmul_nbits_decode.hip): MatMulNBits
for 1 ... 16 rows of A, streamed from the blob into registers (vector ALU; matrix cores for the 8- and 16-row tiers of suitable groups).

1. Exact on integer data: `torch.equal` to the float64 product rounded once to Y's type.  Each case asserts from its own operands
   that every partial sum is exact in fp32 in any order (DecodeCase.exact_in_fp32), so the verdict does not depend on the kernel's
   summation order, and asserts the launch plan it claims with the workspace query for that plan.
2. Random data: |Y - Y64| <= c 2^-24 S + ulp_out / 2 (|Y64| + that), c = g + blocks + 8 (DESIGN.md 4.26 derives it); the relative
   Frobenius error is at most that of the expansion route of `GraphRunner._op_MatMulNBits`.
3. Equal bytes with the tile route (`ops.matmul_nbits`) where both take the node.
4. Refusals name their reason and touch no output.
5. No expanded weight is allocated."""
import pytest
import torch

from nbits_cases import ATYPE, DTYPES, gen
from nbits_decode_cases import ZP_FORMS, DecodeCase, DecodePlan, decode_plan, decode_workspace, raw_decode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from onnx_quantize_amd.hip import ops
    return ops


@pytest.fixture(scope="module")
def lib():
    from onnx_quantize_amd.hip import _lib
    return _lib.load()


def assert_plan(lib, c, expected):
    pl = c.plan()
    assert pl == expected, (c.M, c.K, c.N, pl, expected)
    assert lib.oq_matmul_nbits_decode_workspace_bytes(c.M, c.K, c.N, c.group, ATYPE[c.dtype]) == decode_workspace(c.M, c.K, c.N)
    assert decode_workspace(c.M, c.K, c.N) == (0 if expected.splits == 1 else -(-expected.splits * c.M * c.N * 4 // 256) * 256)
    return pl


# ------------------------------------------------------------------------------------ 1. exact on integer data
# (M, K, N, g), DecodePlan(tier, splits, rows_per_block, row_blocks, grid, k of the last slice), what the row adds
SWEEP = [
    ((1, 7, 1, 16), DecodePlan(1, 1, 64, 1, 1, 7), "K below one lane's unit, one output"),
    ((2, 16, 2, 16), DecodePlan(4, 1, 64, 1, 1, 16), "one unit, g = 16"),
    ((3, 40, 100, 16), DecodePlan(4, 1, 64, 2, 2, 40), "an odd block count (pad nibble), 4-bit rows of 24 bytes: 8-byte loads, a tail group of 8"),
    ((4, 96, 130, 96), DecodePlan(4, 1, 64, 3, 3, 96), "g = K, no power of two"),
    ((5, 100, 257, 32), DecodePlan(8, 1, 64, 5, 5, 100), "a tail group of 4 behind 0xFF padding"),
    ((8, 160, 100, 64), DecodePlan(8, 1, 64, 2, 2, 160), "a tail group of 32 at g = 64, three blocks"),
    ((9, 1088, 130, 128), DecodePlan(16, 2, 64, 3, 6, 64), "two slices, the last of 64"),
    ((16, 1088, 257, 256), DecodePlan(16, 2, 64, 5, 10, 64), "a tail group of 64 at g = 256, five blocks"),
    ((16, 2600, 100, 48), DecodePlan(16, 3, 64, 2, 6, 552), "three slices, a short last one, slice boundaries inside a group of 48"),
    ((1, 2600, 130, 1088), DecodePlan(1, 3, 64, 3, 9, 552), "the one-row tier over three slices, groups longer than a slice"),
    ((4, 1088, 2, 1088), DecodePlan(4, 2, 64, 1, 2, 64), "g = K over two slices"),
    ((8, 64, 1100, 32), DecodePlan(8, 1, 64, 18, 18, 64), "many row blocks"),
    # the matrix-core kernel of the 8- and 16-row tiers (groups of whole wave spans: g % 128 == 0 at 4 bits, g % 64 == 0 at 8 bits)
    ((5, 200, 40, 128), DecodePlan(8, 1, 64, 1, 1, 200), "matrix cores: a tail group of 72, lanes past K, a row tile with a tail of 8"),
    ((12, 1500, 50, 256), DecodePlan(16, 2, 64, 1, 2, 476), "matrix cores: two slices, spans past K skipped"),
    ((16, 1024, 130, 128), DecodePlan(16, 1, 64, 3, 3, 1024), "matrix cores: a whole slice in one launch, a row block with a tail of 2"),
    ((16, 2176, 70, 1088), DecodePlan(16, 3, 64, 2, 6, 128), "VALU: g = 1088 is no whole number of spans"),
    ((9, 3072, 33, 384), DecodePlan(16, 3, 64, 1, 3, 1024), "matrix cores: groups of three spans, a group across a slice boundary"),
]
FORMS = [(zp, native) for native in (False, True) for zp in ZP_FORMS]      # 8: zero points x scales (fp32 / A's type)


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_integers_over_the_plan_sweep(ops, lib, dt, bits):
    """Integers |a| <= 4, scales in {1/8, 1/2, 1}, integer bias, padded positions all-ones, the forced extreme (q, zp) pairs; float
    zero points are multiples of 0.5.  The eight forms of (zero points, scales) rotate over the shapes, starting at another
    one per (type, bits): every (A type, bits, zero points, scales) occurs.  Bias alternates.  All cases run; failures are reported
    together."""
    dtype = DTYPES[dt]
    g = gen(2600 + bits)
    start = sorted(DTYPES).index(dt) * 3 + bits // 8
    failures, seen = [], set()
    for i, (shape, expected, adds) in enumerate(SWEEP):
        zp, native = FORMS[(i + start) % len(FORMS)]
        seen.add((zp, native))
        M, K, N, group = shape
        c = DecodeCase(g, M, K, N, group, bits, dtype, zp=zp, integer=True, bias=i % 2 == 0, scale_dtype=dtype if native else torch.float32)
        assert_plan(lib, c, expected)
        assert c.exact_in_fp32(), shape
        y = c.run(ops)
        assert y.shape == (M, N) and y.dtype == dtype
        wrong = y != c.rounded(c.y64())
        if wrong.any():
            rows, cols = torch.nonzero(wrong, as_tuple=True)
            failures.append(f"{shape} zp={zp} scales={'A' if native else 'fp32'} ({adds}): {int(wrong.sum())} wrong, rows "
                            f"{sorted(set(rows.tolist()))[:8]}, columns {sorted(set(cols.tolist()))[:8]}")
    assert len(seen) == len(FORMS)
    assert not failures, "\n" + "\n".join(failures)


@pytest.mark.parametrize("zp", ZP_FORMS)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_strided_and_odd_offset_operands_give_the_same_bytes(ops, lib, dt, zp):
    """lda > K with an odd element offset of A's base (narrow loads), and ldy > N through the entry point with a sentinel behind N."""
    dtype = DTYPES[dt]
    M, K, N, group = 5, 200, 70, 32
    c = DecodeCase(gen(2611), M, K, N, group, 4, dtype, zp=zp, integer=True)
    assert c.exact_in_fp32()
    want = c.rounded(c.y64())
    assert torch.equal(c.run(ops), want)
    wide = torch.full((M, K + 5), 3.0, device="cuda", dtype=dtype)
    wide[:, 1:1 + K] = c.x
    view = wide[:, 1:1 + K]
    assert view.data_ptr() % 16 == dtype.itemsize                 # the base is off by one element
    assert torch.equal(c.run(ops, view), want)
    ldy = N + 3
    out = torch.full((M, ldy), -77.0, device="cuda", dtype=dtype)
    st, msg = raw_decode(lib, c, out, ldy, x=view, lda=K + 5)
    assert st == 0, msg
    assert torch.equal(out[:, :N], want) and bool((out[:, N:] == -77.0).all())


@pytest.mark.parametrize("M", [16, 1])
def test_a_grid_of_several_workgroups_per_compute_unit_is_exact_and_repeats(ops, lib, M):
    """K = 128, N = 65536: 512 workgroups, two per compute unit, every SIMD shared by waves of several workgroups; 128 rows per
    workgroup, so every wave of the matrix-core kernel (M = 16) walks two tiles, the second one loaded ahead.  Four runs, equal
    bytes, and exact."""
    K, N, group = 128, 65536, 128
    c = DecodeCase(gen(2620), M, K, N, group, 4, torch.float16, zp="packed", integer=True)
    assert_plan(lib, c, DecodePlan(16 if M == 16 else 1, 1, 128, 512, 512, 128))
    assert c.exact_in_fp32()
    want = c.rounded(c.y64())
    runs = [c.run(ops) for _ in range(4)]
    for y in runs:
        assert torch.equal(y, want), int((y != want).sum())


def test_an_fp32_a_in_the_row_tiers_8_and_16_plans_for_one_workgroup_per_compute_unit(ops, lib):
    """N = 20000, K = 128: 64-row blocks for fp16 (313 workgroups of 512 wanted), 128-row blocks for fp32 at M = 16 (157 of 256
    wanted) -- and the fp32 case, two tiles per wave on three bf16 pieces, is exact."""
    assert decode_plan(16, 128, 20000, torch.float16) == DecodePlan(16, 1, 64, 313, 313, 128)
    assert decode_plan(4, 128, 20000, torch.float32) == DecodePlan(4, 1, 64, 313, 313, 128)
    c = DecodeCase(gen(2625), 16, 128, 20000, 128, 4, torch.float32, zp="fp32", integer=True)
    assert_plan(lib, c, DecodePlan(16, 1, 128, 157, 157, 128))
    assert c.exact_in_fp32()
    assert torch.equal(c.run(ops), c.rounded(c.y64()))


# ------------------------------------------------------------------------------------ 2. random data
RANDOM = [(1, 1100, 130, 128), (4, 520, 257, 16), (16, 2600, 100, 64), (8, 96, 70, 96), (9, 1100, 70, 128)]      # the last: matrix cores at 4 bits


def frobenius(y, y64):
    return ((y.to(torch.float64) - y64).norm() / y64.norm()).item()


@pytest.mark.parametrize("zp", ZP_FORMS)
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_random_data_holds_the_bound_and_is_no_worse_than_the_expansion_route(ops, dt, bits, zp):
    dtype = DTYPES[dt]
    g = gen(2630 + bits)
    for M, K, N, group in RANDOM:
        c = DecodeCase(g, M, K, N, group, bits, dtype, zp=zp, scale_dtype=dtype if zp == "native" else torch.float32)
        y, y64 = c.run(ops), c.y64()
        err, bound = (y.to(torch.float64) - y64).abs(), c.bound()
        worst = (err / bound).max().item()
        decode, expansion = frobenius(y, y64), frobenius(c.parent(), y64)
        print(f"{dt} bits={bits} zp={zp} {(M, K, N, group)}: err / bound {worst:.3f}, Frobenius decode {decode:.3e} expansion {expansion:.3e}")
        assert worst <= 1.0, (M, K, N, group, worst)
        assert decode <= expansion, (M, K, N, group, decode, expansion)


@pytest.mark.parametrize("zp", ["packed", "fp32"])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_rows_at_1e30_and_1e_minus_30_hold_the_bound(ops, dt, zp):
    dtype = DTYPES[dt]

    def rows(g, M, K, dt_):
        a = torch.randn((M, K), device="cuda", generator=g)
        a[0] *= 1e30
        a[1] *= 1e-30
        return a.to(dt_)

    c = DecodeCase(gen(2640), 4, 1100, 130, 128, 4, dtype, zp=zp, bias=False, a_values=rows)
    y, y64 = c.run(ops), c.y64()
    assert bool(torch.isfinite(y).all())
    assert ((y.to(torch.float64) - y64).abs() <= c.bound()).all()


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_a_nan_in_one_row_of_a_gives_exactly_that_nan_row(ops, dt):
    c = DecodeCase(gen(2650), 16, 1100, 130, 128, 4, DTYPES[dt], zp="fp32")
    clean = c.run(ops)
    x = c.x.clone()
    x[5, 1030] = float("nan")
    y = c.run(ops, x)
    assert bool(torch.isnan(y[5]).all())
    keep = [m for m in range(16) if m != 5]
    assert torch.equal(y[keep], clean[keep])


# ------------------------------------------------------------------------------------ 3. agreement with the tile route
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_integer_data_gives_the_bytes_of_the_tile_route(ops, dt, bits):
    for M, K, N, group, zp in [(1, 256, 130, 32, "packed"), (16, 1088, 257, 64, "none"), (16, 200, 100, 128, "packed"), (1, 2600, 70, 160, "none")]:
        c = DecodeCase(gen(2660 + bits), M, K, N, group, bits, DTYPES[dt], zp=zp, integer=True)
        assert c.exact_in_fp32()
        assert torch.equal(c.run(ops), c.tile(ops)), (M, K, N, group)


# ------------------------------------------------------------------------------------ 4. refusals
def test_refusals_through_ops_name_their_reason(ops):
    c = DecodeCase(gen(2670), 16, 96, 8, 32, 4, torch.float16, zp="packed", integer=True)
    kw = dict(K=c.K, N=c.N, bits=4, block_size=32)
    with pytest.raises(NotImplementedError, match="17 rows"):
        ops.matmul_nbits_decode(torch.zeros((17, c.K), device="cuda", dtype=torch.float16), c.blob, c.scales, c.zero_points, **kw)
    with pytest.raises(NotImplementedError, match="g_idx"):
        ops.matmul_nbits_decode(c.x, c.blob, c.scales, c.zero_points, g_idx=torch.zeros(c.K, dtype=torch.int32, device="cuda"), **kw)
    with pytest.raises(NotImplementedError, match="bits = 2"):
        ops.matmul_nbits_decode(c.x, c.blob, c.scales, c.zero_points, **{**kw, "bits": 2})
    with pytest.raises(NotImplementedError, match="block_size = 24"):
        ops.matmul_nbits_decode(c.x, c.blob, c.scales, c.zero_points, **{**kw, "block_size": 24})
    assert ops.matmul_nbits_decode_unsupported(torch.float16, 4, 16, torch.zeros(3, device="cuda")) is None       # float zero points, g = 16
    assert ops.matmul_nbits_unsupported(torch.float16, 4, 16) is not None                                         # the twin keeps its refusals
    assert "float zero points" in ops.matmul_nbits_unsupported(torch.float16, 4, 32, torch.zeros(3))


def test_refusals_of_the_entry_point_leave_the_sentinel(lib):
    c = DecodeCase(gen(2671), 16, 96, 8, 32, 4, torch.float16, zp="packed", integer=True)
    big = torch.zeros((17, c.K), device="cuda", dtype=torch.float16)
    for over, word in ((dict(x=big, M=17), "M = 17"), (dict(flags=2), "g_idx"), (dict(bits=2), "bits = 2"), (dict(group=24), "group_size = 24")):
        out = torch.full((17, c.N), -77.0, device="cuda", dtype=torch.float16)
        st, msg = raw_decode(lib, c, out, c.N, **over)
        assert st == -2 and word in msg, (over, st, msg)
        assert bool((out == -77.0).all()), over


# ------------------------------------------------------------------------------------ 5. no expanded weight
def test_no_expanded_weight_is_ever_allocated(ops):
    M, K, N = 1, 1024, 1024
    c = DecodeCase(gen(2680), M, K, N, 128, 4, torch.float16, zp="fp32")

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

    c.run(ops)
    decode, expanded = growth(lambda: c.run(ops)), growth(c.parent)
    print(f"peak growth decode {decode} B, expansion route {expanded} B, fp16 weight {N * K * 2} B")
    assert decode < expanded and decode < N * K * 2
    assert expanded > N * K * 2
