"""`ops.qdq_matmul` / `oq_qdq_matmul` (include/oq_hip_qdq.h, csrc/qdq_matmul.hip): the product of a `quant`-domain QDQ function run
from the [K, N] byte matrix the file stores.  The reference value everywhere is float64:
w64[k, n] = (q - zp[i]) * float64(scale[i]),  Y64 = A64 . w64 + bias64.

1  exact integers: data on which every fp32 operation of any summation order is exact -> torch.equal to Y64 rounded once.
2  random data against the DERIVED bound of test_matmul_nbits_gpu.py (blocks = K / g, or 1 per tensor / per column), and beside
   the expansion route the function body takes today.
3  special values.   4  no expanded weight in memory.   5  refusals leave Y untouched.
"""
import itertools

import pytest
import torch

from nbits_cases import plan
from qdq_cases import ATYPE, DTYPES, Case, describe, gen

pytestmark = pytest.mark.gpu
WDTYPES = (torch.uint8, torch.int8)


@pytest.fixture(scope="module")
def ops():
    from onnx_quantize_amd.hip import ops
    return ops


@pytest.fixture(scope="module")
def lib():
    from onnx_quantize_amd.hip import _lib
    return _lib


# ------------------------------------------------------------------------------------ 1. exact integers
# |A| <= 4 integers, |q - zp| <= 255, scales in {1/8, 1/2, 1}, K <= 1280: every partial sum is a multiple of 1/8 below 2^24 / 8, exact
# in fp32 in any order -- the result IS the float64 value rounded once to A's type.
# M in {1, 31, 33, 129} x K in {1, 63, 64, 65, 200} x N in {1, 3, 127, 129, 260}: every value with every other at least once
FLAT_SHAPES = [(1, 1, 1), (31, 63, 3), (33, 64, 127), (129, 65, 129), (33, 200, 260), (1, 200, 129), (129, 64, 260), (31, 65, 1),
               (129, 1, 127), (1, 63, 260), (31, 64, 129), (33, 65, 3), (129, 200, 1), (1, 64, 3), (31, 200, 127), (33, 63, 1),
               (129, 63, 129), (31, 1, 260), (33, 1, 3), (1, 65, 127)]


@pytest.mark.parametrize("granularity", ["tensor", "column"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_integers_per_tensor_and_per_column(ops, dt, granularity):
    g = gen(100)
    options = itertools.cycle(itertools.product(WDTYPES, (True, False), (True, False)))      # W's type, zero points, bias
    for (M, K, N), (wdtype, zero_points, bias) in zip(FLAT_SHAPES * 2, options):              # 40 cases over the 8 combinations
        c = Case(g, M, K, N, granularity, DTYPES[dt], wdtype, zero_points=zero_points, bias=bias, integer=True)
        wrong = c.run(ops) != c.rounded(c.y64())
        assert not wrong.any(), ((M, K, N), wdtype, zero_points, bias, describe(wrong, c.plan()))


# K = 576 (groups of 32, 64) and 1280 (groups of 128) with at most 32 rows and 2 tiles: 8 splits are wanted, the last one is short
GROUP_SHAPES = {32: [(33, 64, 127), (1, 256, 260), (31, 576, 3), (129, 256, 129)], 64: [(129, 64, 129), (31, 256, 1), (1, 576, 127), (33, 256, 260)],
                128: [(33, 256, 260), (31, 1280, 129), (129, 256, 3), (1, 1280, 1)]}


@pytest.mark.parametrize("group", sorted(GROUP_SHAPES))
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_integers_per_group(ops, dt, group):
    g = gen(200 + group)
    plans = [plan(*shape) for shape in GROUP_SHAPES[group]]
    assert any(pl.splits > 1 and pl.last < pl.steps_per_split for pl in plans), "no shape whose last split is short"
    options = itertools.cycle(itertools.product(WDTYPES, (True, False), (True, False)))
    for (M, K, N), (wdtype, zero_points, bias) in zip(GROUP_SHAPES[group] * 2, options):
        c = Case(g, M, K, N, group, DTYPES[dt], wdtype, zero_points=zero_points, bias=bias, integer=True)
        wrong = c.run(ops) != c.rounded(c.y64())
        assert not wrong.any(), ((M, K, N), wdtype, zero_points, bias, describe(wrong, c.plan()))


@pytest.mark.parametrize("granularity", ["column", 32])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_integers_on_a_grid_of_512_workgroups_four_times(ops, lib, dt, granularity):
    """512 tiles of 128 rows, K in one step (no slabs): more workgroups than the 256 CUs, so waves of different workgroups share a
    SIMD.  A build of matmul_nbits.hip whose per-group fold was paired into v_pk_fma_f32 got exactly this wrong, differently from
    run to run, while every smaller grid passed (docs/LAB_NOTES_r22.md): four calls, exact, equal bytes."""
    M, K, N = 1024, 64, 8192
    c = Case(gen(13), M, K, N, granularity, DTYPES[dt], torch.int8, integer=True)
    pl = c.plan()
    assert pl.tiles >= 512 and pl.splits == 1, pl
    assert lib.load().oq_qdq_matmul_workspace_bytes(M, K, N, ATYPE[c.dtype]) == c.workspace()
    want = c.rounded(c.y64())
    wrong = [c.run(ops) != want for _ in range(4)]
    for i, w in enumerate(wrong):
        if w.any():
            print(f"call {i}: {describe(w, pl)}")
    assert [int(w.sum()) for w in wrong] == [0, 0, 0, 0]


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_views_with_gaps_odd_bases_and_every_alignment_of_w_give_the_same_bytes(ops, lib, dt):
    """lda > K with NaNs in the gap, an A whose base sits at an odd element offset, W at every base alignment mod 4 with rows at
    every alignment (ldw odd) and with aligned rows and a gap (ldw % 4 == 0), the gaps of W full of garbage, and ldy > N through the
    C ABI with the gap columns of Y keeping their sentinel."""
    dtype = DTYPES[dt]
    for (M, K, N), granularity in (((33, 200, 127), "column"), ((3, 256, 17), 64), ((17, 65, 260), "tensor")):
        c = Case(gen(11), M, K, N, granularity, dtype, torch.uint8, integer=True)
        want = c.rounded(c.y64())
        wide = torch.full((M, K + 24), float("nan"), device="cuda", dtype=dtype)
        wide[:, :K] = c.x
        assert torch.equal(c.run(ops, wide[:, :K]), want)                     # lda = K + 24
        odd = torch.full((M * (K + 3) + 1,), float("nan"), device="cuda", dtype=dtype)
        view = odd[1:].reshape(M, K + 3)[:, :K]
        view.copy_(c.x)
        assert view.data_ptr() % 16 != 0 and torch.equal(c.run(ops, view), want)
        for offset, ldw in itertools.chain(((o, N + (1 - N) % 4) for o in range(4)), ((0, N + (-N) % 4 + 8),)):
            flat = torch.randint(0, 256, (offset + K * ldw + 3,), device="cuda", generator=gen(offset), dtype=torch.int32).to(torch.uint8)
            w = flat[offset:offset + K * ldw].reshape(K, ldw)[:, :N]
            w.copy_(c.w)
            assert w.data_ptr() % 4 == offset and w.stride(0) == ldw
            wrong = c.run(ops, w=w) != want
            assert not wrong.any(), (offset, ldw, describe(wrong, c.plan()))
        y = torch.full((M, N + 5), -77.0, device="cuda", dtype=dtype)         # ldy > N: straight through the library
        assert c.raw(lib, y, N + 5, x=wide, lda=K + 24) == 0, lib.load().oq_last_error()
        assert torch.equal(y[:, :N], want) and (y[:, N:] == -77.0).all()


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_the_same_call_twice_gives_the_same_bytes(ops, dt):
    for (M, K, N), granularity in (((70, 1024, 260), 128), ((3, 4096, 64), "column")):      # one pass over K, and K split across workgroups
        c = Case(gen(5), M, K, N, granularity, DTYPES[dt], torch.int8)
        first, second = c.run(ops), c.run(ops)
        assert torch.equal(first.view(torch.uint8), second.view(torch.uint8))


# ------------------------------------------------------------------------------------ 2. random data
def rel_fro(y, y64):
    return ((y.to(torch.float64) - y64).norm() / y64.norm()).item()


@pytest.mark.parametrize("scales", ["fp32 scales", "scales of A's type"])
@pytest.mark.parametrize("shape", [(70, 1024, 260), (3, 4096, 64)], ids=str)
@pytest.mark.parametrize("granularity", ["tensor", "column", 128])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_random_data_stays_inside_the_derived_bound_and_beside_the_expansion_route(ops, dt, granularity, shape, scales):
    """|Y - Y64| <= Case.bound(), the derivation of nbits_cases with blocks = K / g (1 per tensor / per column).  The relative
    Frobenius error is printed beside the expansion route's; for a 2-byte A the expansion rounds the weight to A's type and
    accumulates as torch's GEMM does, and the fused product must not be the less accurate of the two."""
    M, K, N = shape
    dtype = DTYPES[dt]
    wdtype = torch.int8 if granularity == "column" else torch.uint8
    c = Case(gen(21), M, K, N, granularity, dtype, wdtype, scale_dtype=torch.float32 if scales == "fp32 scales" else dtype)
    y, y64 = c.run(ops), c.y64()
    assert y.dtype == dtype and y.shape == (M, N)
    excess = ((y.to(torch.float64) - y64).abs() - c.bound()).max().item()
    ours, parents = rel_fro(y, y64), rel_fro(c.parent(), y64)
    print(f"{dt} {granularity} {shape} {scales}: max(|err| - bound) = {excess:.3e}, rel. Frobenius {ours:.3e} (expansion route {parents:.3e})")
    assert excess <= 0.0
    if dtype != torch.float32:
        assert ours <= parents


@pytest.mark.parametrize("factor", [1e30, 1e-30])
def test_fp32_rows_of_any_magnitude_keep_the_relative_bound(ops, factor):
    c = Case(gen(31), 70, 1024, 260, 128, torch.float32, bias=False)
    x = c.x * factor
    x[1::2] = c.x[1::2]                                                    # neighbours of ordinary size: every row has its own scale
    y, y64 = c.run(ops, x), c.y64(x)
    assert torch.isfinite(y).all()
    assert (((y.to(torch.float64) - y64).abs() - c.bound(x)).max().item()) <= 0.0


# ------------------------------------------------------------------------------------ 3. special values
@pytest.mark.parametrize("shape", [(70, 1024, 260), (3, 4096, 64)], ids=str)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_a_nan_poisons_exactly_its_row(ops, dt, shape):
    M, K, N = shape
    c = Case(gen(41), M, K, N, "column", DTYPES[dt], torch.int8)
    clean = c.run(ops)
    x = c.x.clone()
    x[2, K - 3] = float("nan")
    y = c.run(ops, x)
    assert torch.isnan(y[2]).all()
    keep = [m for m in range(M) if m != 2]
    assert torch.equal(y[keep], clean[keep])


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_a_zero_input_gives_exactly_the_bias(ops, dt):
    c = Case(gen(43), 19, 320, 45, 64, DTYPES[dt])
    y = c.run(ops, torch.zeros_like(c.x))
    assert torch.equal(y, c.bias.expand(19, 45))


# ------------------------------------------------------------------------------------ 4. no expanded weight
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_no_expanded_weight_is_ever_allocated(ops, dt):
    M, K, N = 16, 1024, 1024
    c = Case(gen(51), M, K, N, 128, DTYPES[dt])

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

    c.run(ops)                                                             # the library is loaded, its workspace sizes are known
    fused, expanded = growth(lambda: c.run(ops)), growth(c.parent)
    print(f"{dt}: peak growth fused {fused} B, expansion route {expanded} B, fp32 weight {N * K * 4} B")
    assert fused < K * N * 4
    assert expanded > K * N * 4                                            # the route it replaces does pay it: the test is not vacuous


# ------------------------------------------------------------------------------------ 5. refusals
def test_refusals_leave_y_untouched_and_the_op_raises_by_name(ops, lib):
    c = Case(gen(61), 8, 256, 16, 32, torch.float16, bias=False, integer=True)      # K in four steps: slabs, so a workspace
    y = torch.full((8, 16), -77.0, device="cuda", dtype=torch.float16)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    raw = lib.load()
    for kw, status, word in ((dict(group_size=16), -2, "group_size = 16"), (dict(group_size=48), -2, "group_size = 48"),
                             (dict(group_size=0), -2, "group_size = 0"), (dict(K=96, lda=96, group_size=64), -2, "no multiple of group_size"),
                             (dict(atype=5), -1, "atype"), (dict(wtype=0), -1, "wtype"), (dict(granularity=3), -1, "granularity"),
                             (dict(lda=255), -1, "lda=255"), (dict(ldw=15), -1, "ldw=15"), (dict(M=0), -1, "M=0"),
                             (dict(workspace_bytes=64), -3, "workspace")):
        assert c.raw(lib, y, 16, workspace=ws, **kw) == status, (kw, raw.oq_last_error())
        assert word in raw.oq_last_error().decode(), (kw, raw.oq_last_error())
    assert c.raw(lib, y, 15, workspace=ws) == -1 and "ldy=15" in raw.oq_last_error().decode()
    torch.cuda.synchronize()
    assert (y == -77.0).all()
    assert c.raw(lib, y, 16, workspace=ws) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, c.rounded(c.y64()))

    with pytest.raises(NotImplementedError, match="group_size = 16"):
        ops.qdq_matmul(c.x, c.w, c.scales, c.zero_points, group_size=16)
    with pytest.raises(NotImplementedError, match="float64"):
        ops.qdq_matmul(c.x.double(), c.w, c.scales, c.zero_points, group_size=32)
    with pytest.raises(NotImplementedError, match="zero point of torch.int8"):
        ops.qdq_matmul(c.x, c.w, c.scales, c.zero_points.to(torch.int8), group_size=32)
    with pytest.raises(NotImplementedError, match="scales for"):
        ops.qdq_matmul(c.x, c.w, c.scales[:5], None)
    assert ops.qdq_matmul_unsupported(c.x, c.w, c.scales, c.zero_points, group_size=32) is None


def test_leading_axes_are_flattened_and_restored(ops):
    c = Case(gen(71), 24, 96, 40, "column", torch.float16, torch.int8, integer=True)
    y = c.run(ops, c.x.reshape(2, 3, 4, 96))
    assert y.shape == (2, 3, 4, 40) and torch.equal(y.reshape(24, 40), c.rounded(c.y64()))
