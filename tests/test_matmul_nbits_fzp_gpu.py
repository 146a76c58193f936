"""`ops.matmul_nbits_float_zp` / `oq_matmul_nbits_fzp` (include/oq_hip_nbits_fzp.h, csrc/matmul_nbits_fzp.hip): a MatMulNBits node
with floating-point zero points (an HQQ file) run from its packed blob at any number of rows.  The reference value everywhere is
float64:  w64 = (q - zp) * float64(scale) with zp the stored float,  Y64 = A64 . w64^T + bias64.

1  exact integers: data on which every fp32 operation of any summation order is exact -> torch.equal to Y64 rounded once.
2  ties to the existing kernels: whole zero points give the bytes of `ops.matmul_nbits`, integer data those of the decode route.
3  random data against the DERIVED bound of DESIGN.md 4.30, and against the expansion route of `GraphRunner._op_MatMulNBits`.
4  poisoning: a NaN of A its row, a NaN zero point its column.   5  memory and refusals.
"""
import pytest
import torch

from nbits_cases import ATYPE, DTYPES, Plan, describe, gen
from nbits_fzp_cases import FzpCase, raw_fzp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from onnx_quantize_amd.hip import ops
    return ops


@pytest.fixture(scope="module")
def lib():
    from onnx_quantize_amd.hip import _lib
    return _lib


def planted(N, blocks, top):
    """Zero points outside [0, top], below and above, in the first and in the last group of the last column (of one group: above)."""
    return ((N - 1, 0, -3.5), (N - 1, blocks - 1, top + 4.5))


def exact_case(g, M, K, N, group, bits, dtype, zp, **kw):
    """An integer case with its planted cells, its precondition asserted: S' < 2^24 quanta of 2^-4."""
    blocks, top = -(-K // group), (1 << bits) - 1
    c = FzpCase(g, M, K, N, group, bits, dtype, zp=zp, integer=True, plant=planted(N, blocks, top), **kw)
    assert c.exact_in_fp32(), (M, K, N, group, bits, c.magnitude().max().item())
    zi, f = c.split()
    assert (f.abs() > 0.5).any()                                         # what a clamp cut off
    assert N == 1 or (f[0, 0] == 0.5 and zi[0, 0] == 2.0)                # a tie of rint, to even (column 0: no planted cell)
    return c


# ------------------------------------------------------------------------------------ 1. exact integers
MS, NS = (1, 17, 32, 33, 129), (1, 127, 129, 260)
KS = {4: (72, 200, 1088, 1280), 8: (72, 200, 512)}                       # 8 bits: K <= 512 keeps (255 + 4.5) * 4 * K below 2^20
GROUPS = (32, 64, 96, 128, 256)


def exact_shapes(bits):
    """(group, M, K, N): every group size with every K, g = K where that is a multiple of 32; M and N rotate through their values
    (5 and 4 of them: 20 distinct pairs)."""
    shapes = [(group, K) for group in GROUPS for K in KS[bits]] + [(K, K) for K in (32,) + KS[bits][2:]]
    return [(group, MS[i % 5], K, NS[i % 4]) for i, (group, K) in enumerate(shapes)]


@pytest.mark.parametrize("zp", ["fp32", "native"])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_integers_over_the_grid(ops, dt, bits, zp):
    """|A| <= 4 integers, scales in {1/8, 1/2, 1}, zero points multiples of 1/2 (half of them ties of rint), two cells outside
    the range: every partial sum -- acc, rs, f * rs, the scaled sums -- is a multiple of 2^-4 below 2^24 of them, exact in fp32 in
    any order, so the result IS the float64 value rounded once to A's type.  The table reaches both tiles and a partial row tile,
    two groups inside one k-step (g = 32), a group boundary in the middle of a step (g = 96), a tail group, K % 32 != 0 and
    K % 8 != 0, a split K with a short last split and a split boundary inside a group (asserted from the plan)."""
    g = gen(300 + bits)
    bad, seen = [], set()
    shapes = exact_shapes(bits)
    assert {s[1] for s in shapes} == set(MS) and {s[3] for s in shapes} == set(NS)
    for i, (group, M, K, N) in enumerate(shapes):
        c = exact_case(g, M, K, N, group, bits, DTYPES[dt], zp, bias=i % 2 == 0)
        pl = c.plan()
        if pl.splits > 1 and (pl.steps_per_split * 64) % group:
            seen.add("a split boundary inside a group" + (", g = K" if group == K else ", g = 256" if group == 256 else ""))
        if pl.splits > 1 and pl.last < pl.steps_per_split:
            seen.add("a short last split")
        if K % group:
            seen.add("a tail group")
        seen.add(f"{pl.bm}-row tile")
        wrong = c.run(ops) != c.rounded(c.y64())
        if wrong.any():
            bad.append(((group, M, K, N), describe(wrong, pl)))
    reached = {"a split boundary inside a group, g = K", "a split boundary inside a group, g = 256", "a tail group", "32-row tile", "128-row tile"}
    if bits == 4:                                                        # K <= 512 is at most 8 k-steps: every split is one step
        reached.add("a short last split")
    assert reached <= seen, seen
    assert not bad, bad


# (shape, bits, g): 512 tiles of each tile height, the plans of test_matmul_nbits_gpu.py
LARGE_GRID_PLANS = {(2048, 256, 4096): Plan(128, 16, 32, 4, 4, 1, 4), (16, 256, 65536): Plan(32, 1, 512, 4, 4, 1, 4)}
LARGE_GRIDS = [(shape, bits, group) for shape in LARGE_GRID_PLANS for bits, group in ((4, 128), (8, 32))]


@pytest.mark.parametrize("case", LARGE_GRIDS, ids=[f"{s}-{b}bit-g{g}" for s, b, g in LARGE_GRIDS])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_integers_on_grids_of_several_workgroups_per_cu(ops, lib, dt, case):
    """512 tiles, K in one pass: more workgroups than compute units, so waves of different workgroups share a SIMD -- where a paired
    fold went wrong in the integer kernel (docs/LAB_NOTES_r22.md).  This fold has two fmas per element: four calls, exact, and
    the same bytes each time."""
    (M, K, N), bits, group = case
    c = exact_case(gen(13), M, K, N, group, bits, DTYPES[dt], "fp32")
    pl = c.plan()
    assert pl == LARGE_GRID_PLANS[(M, K, N)] and pl.tiles >= 512, pl
    assert lib.load().oq_matmul_nbits_fzp_workspace_bytes(M, K, N, group, ATYPE[c.dtype]) == c.workspace()
    want = c.rounded(c.y64())
    wrong = [c.run(ops) != want for _ in range(4)]
    for i, w in enumerate(wrong):
        if w.any():
            print(f"call {i}: {describe(w, pl)}")
    assert [int(w.sum()) for w in wrong] == [0, 0, 0, 0]


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_views_with_gaps_and_an_odd_base_give_the_same_bytes(ops, lib, dt):
    """lda > K, an A whose base sits at an odd element offset (rows no longer 16-byte aligned: narrower loads), ldy > N through the
    C ABI with the gap columns of Y keeping their sentinel, and split K (M = 3, K = 256: slabs)."""
    dtype = DTYPES[dt]
    for M, K, N in ((33, 256, 100), (3, 256, 17), (17, 100, 40)):
        c = exact_case(gen(11), M, K, N, 32, 4, dtype, "native")
        want = c.rounded(c.y64())
        wide = torch.full((M, K + 24), 3.0, device="cuda", dtype=dtype)
        wide[:, :K] = c.x
        assert torch.equal(c.run(ops, wide[:, :K]), want)                     # lda = K + 24
        odd = torch.full((M * (K + 3) + 1,), 3.0, device="cuda", dtype=dtype)
        view = odd[1:].reshape(M, K + 3)[:, :K]
        view.copy_(c.x)
        assert view.data_ptr() % 16 != 0 and torch.equal(c.run(ops, view), want)
        y = torch.full((M, N + 5), -77.0, device="cuda", dtype=dtype)
        st, msg = raw_fzp(lib.load(), c, y, N + 5, x=wide[:, :K])             # lda and ldy straight through the library
        assert st == 0, msg
        assert torch.equal(y[:, :N], want) and (y[:, N:] == -77.0).all()


# ------------------------------------------------------------------------------------ 2. ties to the existing kernels
@pytest.mark.parametrize("M", [33, 129])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_whole_zero_points_give_the_bytes_of_the_integer_kernel(ops, dt, M):
    """Integer-valued float zero points in [0, top]: f = 0, the correction adds a zero, and everything else -- the operand, the
    plan, the order of the fold -- is oq_matmul_nbits': random finite data, equal bytes."""
    for K, N, group, bits, zp, scale_dtype in ((1088, 260, 64, 4, "fp32", torch.float32), (320, 130, 32, 8, "native", DTYPES[dt])):
        c = FzpCase(gen(17), M, K, N, group, bits, DTYPES[dt], zp=zp, values="whole", scale_dtype=scale_dtype)
        assert (c.split()[1] == 0).all() and torch.isfinite(c.x).all()
        ours, theirs = c.run(ops), c.packed(ops)
        assert torch.equal(ours.view(torch.uint8), theirs.view(torch.uint8)), describe(ours != theirs, c.plan())


@pytest.mark.parametrize("M", [1, 5, 16])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_integer_data_gives_the_bytes_of_the_decode_route(ops, dt, M):
    for K, N, group, bits in ((1280, 130, 128, 4), (200, 127, 32, 4), (512, 129, 64, 8)):
        c = exact_case(gen(19), M, K, N, group, bits, DTYPES[dt], "fp32")
        assert torch.equal(c.run(ops).view(torch.uint8), c.decode(ops).view(torch.uint8))


# ------------------------------------------------------------------------------------ 3. random data
RANDOM_SHAPES = [(70, 1024, 260, 128, "fp32"), (17, 2048, 64, 64, "native")]
ZERO_POINTS = {"uniform in the range": dict(), "as HQQ leaves them": dict(values="hqq"),
               "a few outside the range": dict(values="hqq", plant=((0, 0, -2.75), (1, 0, 1e3), (5, 3, -40.125), (63, 7, 300.3)))}


def rel_fro(y, y64):
    return ((y.to(torch.float64) - y64).norm() / y64.norm()).item()


@pytest.mark.parametrize("zero_points", sorted(ZERO_POINTS))
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=[str(s) for s in RANDOM_SHAPES])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_random_data_stays_inside_the_derived_bound_and_beside_the_expansion_route(ops, dt, bits, shape, zero_points):
    """|Y - Y64| <= term + unit (|Y64| + term), term = (K + 3 blocks + 4) 2^-23 S' (DESIGN.md 4.30).  A 2-byte A: no larger a
    relative Frobenius error than the expansion route, which rounds every weight to two bytes where this kernel rounds none."""
    M, K, N, group, zp = shape
    dtype = DTYPES[dt]
    c = FzpCase(gen(21), M, K, N, group, bits, dtype, zp=zp, scale_dtype=torch.float32 if zp == "fp32" else dtype, **ZERO_POINTS[zero_points])
    y, y64 = c.run(ops), c.y64()
    assert y.dtype == dtype and y.shape == (M, N)
    excess = ((y.to(torch.float64) - y64).abs() - c.bound()).max().item()
    ours, parents = rel_fro(y, y64), rel_fro(c.parent(), y64)
    print(f"{dt} bits={bits} {shape} {zero_points}: max(|err| - bound) = {excess:.3e}, rel. Frobenius {ours:.3e} (expansion route {parents:.3e})")
    assert excess <= 0.0
    if dtype != torch.float32:
        assert ours <= parents


@pytest.mark.parametrize("factor", [1e30, 1e-30])
def test_fp32_rows_of_any_magnitude_keep_the_relative_bound(ops, factor):
    c = FzpCase(gen(31), 70, 1024, 260, 128, 4, torch.float32, values="hqq", bias=False)
    x = c.x * factor
    x[1::2] = c.x[1::2]                                                    # neighbours of ordinary size: every row has its own scale
    y, y64 = c.run(ops, x), c.y64(x)
    assert torch.isfinite(y).all()
    assert (((y.to(torch.float64) - y64).abs() - c.bound(x)).max().item()) <= 0.0


# ------------------------------------------------------------------------------------ 4. poisoning
POISON_SHAPES = [(70, 1024, 260), (3, 4096, 64)]                           # one pass over K, and K split across workgroups


@pytest.mark.parametrize("shape", POISON_SHAPES, ids=str)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_a_nan_in_a_poisons_exactly_its_row(ops, dt, shape):
    M, K, N = shape
    c = FzpCase(gen(41), M, K, N, 128, 4, DTYPES[dt], values="hqq")
    clean = c.run(ops)
    assert torch.isfinite(clean).all()
    keep = [m for m in range(M) if m != 2]
    for k in (0, K // 2 + 5, K - 1):
        x = c.x.clone()
        x[2, k] = float("nan")
        y = c.run(ops, x)
        assert torch.isnan(y[2]).all(), k
        assert torch.equal(y[keep], clean[keep]), k


@pytest.mark.parametrize("shape", POISON_SHAPES, ids=str)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_a_nan_zero_point_poisons_exactly_its_column(ops, dt, shape):
    M, K, N = shape
    c = FzpCase(gen(43), M, K, N, 128, 4, DTYPES[dt], values="hqq")
    clean = c.run(ops)
    column, block = N - 3, K // 128 - 2
    c.zero_points[column, block] = float("nan")
    y = c.run(ops)
    assert torch.isnan(y[:, column]).all()
    keep = [n for n in range(N) if n != column]
    assert torch.equal(y[:, keep], clean[:, keep])


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_a_zero_input_gives_exactly_the_bias(ops, dt):
    c = FzpCase(gen(45), 19, 320, 45, 64, 8, DTYPES[dt], values="hqq")
    y = c.run(ops, torch.zeros_like(c.x))
    assert torch.equal(y, c.bias.expand(19, 45))


# ------------------------------------------------------------------------------------ 5. memory and refusals
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_a_call_allocates_its_output_and_its_workspace(ops, lib, dt):
    M, K, N = 64, 1024, 1024
    c = FzpCase(gen(51), M, K, N, 128, 4, DTYPES[dt], values="hqq")

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

    def r512(n):
        return (n + 511) // 512 * 512

    c.run(ops)                                                             # the library is loaded
    need = lib.load().oq_matmul_nbits_fzp_workspace_bytes(M, K, N, 128, ATYPE[c.dtype])
    assert need == c.workspace()
    fused, expanded = growth(lambda: c.run(ops)), growth(c.parent)
    print(f"{dt}: peak growth fused {fused} B (output {M * N * c.x.element_size()} B, workspace {need} B), expansion route {expanded} B")
    assert fused <= r512(M * N * c.x.element_size()) + r512(max(need, 256))
    assert expanded >= N * K * 4                                           # the route it replaces pays for an fp32 [N, K] weight


def test_refusals_leave_y_untouched_and_the_op_raises_by_name(ops, lib):
    c = exact_case(gen(61), 8, 64, 16, 32, 4, torch.float16, "fp32", bias=False)
    raw = lib.load()
    y = torch.full((8, 16), -77.0, device="cuda", dtype=torch.float16)
    packed = torch.zeros(16, dtype=torch.uint8, device="cuda")
    for kw, status, word in ((dict(bits=3), -2, "bits = 3"), (dict(group=16), -2, "group_size = 16"), (dict(group=48), -2, "group_size = 48"),
                             (dict(flags=2), -2, "g_idx"), (dict(flags=3), -2, "g_idx"), (dict(zero_points=packed, zp_type=3), -2, "packed uint8"),
                             (dict(zero_points=None), -2, "NULL"), (dict(zp_type=2), -1, "zero_points_type")):
        st, msg = raw_fzp(raw, c, y, 16, **kw)
        assert st == status and word in msg, (kw, st, msg)
    assert (y == -77.0).all()
    st, msg = raw_fzp(raw, c, y, 16, flags=1)
    assert st == 0, msg
    assert torch.equal(y, c.rounded(c.y64()))

    args = dict(K=64, N=16, bits=4, block_size=32)
    with pytest.raises(NotImplementedError, match="integer zero points"):
        ops.matmul_nbits_float_zp(c.x, c.blob, c.scales, packed, **args)
    with pytest.raises(NotImplementedError, match="integer zero points"):
        ops.matmul_nbits_float_zp(c.x, c.blob, c.scales, None, **args)
    with pytest.raises(NotImplementedError, match="block_size = 16"):
        ops.matmul_nbits_float_zp(c.x, c.blob, c.scales, c.zero_points, **{**args, "block_size": 16})
    with pytest.raises(NotImplementedError, match="bits = 3"):
        ops.matmul_nbits_float_zp(c.x, c.blob, c.scales, c.zero_points, **{**args, "bits": 3})
    with pytest.raises(NotImplementedError, match="zero points of torch.bfloat16"):
        ops.matmul_nbits_float_zp(c.x, c.blob, c.scales, c.zero_points.bfloat16(), **args)
    with pytest.raises(NotImplementedError, match="float64"):
        ops.matmul_nbits_float_zp(c.x.double(), c.blob, c.scales, c.zero_points, **args)
    with pytest.raises(ValueError, match="zero points"):
        ops.matmul_nbits_float_zp(c.x, c.blob, c.scales, c.zero_points[:, :1], **args)
    assert ops.matmul_nbits_float_zp_unsupported(torch.float16, 4, 32, c.zero_points) is None
    assert ops.matmul_nbits_float_zp_unsupported(torch.float16, 4, 32, c.zero_points, g_idx=torch.zeros(64)) == "g_idx"
    assert "float zero points" in ops.matmul_nbits_unsupported(torch.float16, 4, 32, c.zero_points)      # the integer kernel's refusal stays
    with pytest.raises(NotImplementedError, match="float zero points"):
        ops.matmul_nbits(c.x, c.blob, c.scales, c.zero_points, **args)


def test_leading_axes_are_flattened_and_restored(ops):
    c = exact_case(gen(71), 24, 96, 40, 32, 4, torch.float16, "native")
    y = ops.matmul_nbits_float_zp(c.x.reshape(2, 3, 4, 96), c.blob, c.scales, c.zero_points, K=96, N=40, bits=4, block_size=32, bias=c.bias)
    assert y.shape == (2, 3, 4, 40) and torch.equal(y.reshape(24, 40), c.rounded(c.y64()))
