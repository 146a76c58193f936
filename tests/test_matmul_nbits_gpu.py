"""`ops.matmul_nbits` / `oq_matmul_nbits` (include/oq_hip_nbits.h, csrc/matmul_nbits.hip): a MatMulNBits node run from its packed
blob.  The reference value everywhere is float64:  w64 = (q - zp) * float64(scale),  Y64 = A64 . w64^T + bias64.

1  exact integers: data on which every fp32 operation of any summation order is exact -> torch.equal to Y64 rounded once.
2  random data against a DERIVED bound (worst case of an fp32 sum of exact products, a scale multiply per group, one output
   rounding; doubled once for the matrix core's internal order), and against the expansion route of `GraphRunner._op_MatMulNBits`.
3  special values.   4  no expanded weight in memory.   5  refusals leave Y untouched.
"""
import pytest
import torch

from nbits_cases import ATYPE, DTYPES, Case, Plan, describe, gen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from onnx_quantize_amd.hip import ops
    return ops


@pytest.fixture(scope="module")
def lib():
    from onnx_quantize_amd.hip import _lib
    return _lib


# ------------------------------------------------------------------------------------ 1. exact integers
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_integers_over_the_grid(ops, dt, bits):
    """|A| <= 4 integers, scales in {1/8, 1/2, 1}, K <= 256: every partial sum is a multiple of 1/8 below 2^21, exact in fp32 in
    any order -- the result IS the float64 value rounded once to A's type."""
    g = gen(100 + bits)
    bad = []
    for group in (32, 64, 128, 256):
        for zero_points in (False, True):
            for M in (1, 15, 16, 17, 33):
                for N in (1, 16, 17, 100):
                    for K in sorted({group, 256}):
                        c = Case(g, M, K, N, group, bits, DTYPES[dt], zero_points=zero_points, bias=(M + N) % 2 == 0, integer=True)
                        if not torch.equal(c.run(ops), c.rounded(c.y64())):
                            bad.append((group, zero_points, M, N, K))
    assert not bad, bad


@pytest.mark.parametrize("K,group", [(160, 64), (100, 32), (96, 32), (40, 32), (7, 32)])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_integers_with_a_tail_group_and_an_odd_block_count(ops, dt, bits, K, group):
    """K no multiple of g: the blob is padded (every padded byte 0xFF here) and contributes nothing; 160 / 64 and 96 / 32 leave an
    odd block count, whose packed 4-bit zero points end in a pad nibble (0xF here) that is no data."""
    for M, N in ((17, 33), (3, 130)):
        c = Case(gen(7), M, K, N, group, bits, DTYPES[dt], integer=True)
        if K in (160, 96) and bits == 4:
            assert (c.zero_points[:, -1] >> 4 == 0xF).all()
        if K % group and bits == 8:
            assert (c.blob.reshape(N, -1)[:, K:] == 0xFF).all()
        assert torch.equal(c.run(ops), c.rounded(c.y64()))


# (shape, bits, g): 4 bits at g = 128 on the first two shapes are the cases of round 22 and keep their ids
LARGE_GRID_PLANS = {(2048, 256, 4096): Plan(128, 16, 32, 4, 4, 1, 4), (16, 256, 65536): Plan(32, 1, 512, 4, 4, 1, 4),
                    (16, 64, 131072): Plan(32, 1, 1024, 1, 1, 1, 1)}
LARGE_GRIDS = [(shape, bits, group) for shape in LARGE_GRID_PLANS for bits in (4, 8) for group in (128, 32)]


def large_grid_id(case):
    shape, bits, group = case
    return str(shape) if (bits, group) == (4, 128) and shape[1] == 256 else f"{shape}-{bits}bit-g{group}"


@pytest.mark.parametrize("case", LARGE_GRIDS, ids=large_grid_id)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_integers_on_grids_of_several_workgroups_per_cu(ops, lib, dt, case):
    """512 tiles of each tile height, K in one pass (no slabs): more workgroups than the 256 CUs, so waves of different workgroups
    share a SIMD.  A build whose per-group fold was paired into v_pk_fma_f32 got exactly this wrong (rows 12 and 14 of a tile's
    second 16 columns, differently from run to run) while every smaller grid passed (docs/LAB_NOTES_r22.md): four calls, exact.
    Both widths of q, a fold after every MFMA depth (g = 32) as well as one per two steps (g = 128), and 1024 tiles of the 32-row
    kernel with K in one step (16 x 64 x 131072): four workgroups of that kernel fit a CU."""
    (M, K, N), bits, group = case
    c = Case(gen(13), M, K, N, group, bits, DTYPES[dt], integer=True)
    pl = c.plan()
    assert pl == LARGE_GRID_PLANS[(M, K, N)] and pl.tiles >= 512, pl
    assert lib.load().oq_matmul_nbits_workspace_bytes(M, K, N, group, ATYPE[c.dtype]) == c.workspace()
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
        c = Case(gen(11), M, K, N, 32, 4, dtype, integer=True)
        want = c.rounded(c.y64())
        wide = torch.full((M, K + 24), 3.0, device="cuda", dtype=dtype)
        wide[:, :K] = c.x
        assert torch.equal(c.run(ops, wide[:, :K]), want)                     # lda = K + 24
        odd = torch.full((M * (K + 3) + 1,), 3.0, device="cuda", dtype=dtype)
        view = odd[1:].reshape(M, K + 3)[:, :K]
        view.copy_(c.x)
        assert view.data_ptr() % 16 != 0 and torch.equal(c.run(ops, view), want)
        # ldy > N: straight through the library
        raw = lib.load()
        atype = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[dtype]
        y = torch.full((M, N + 5), -77.0, device="cuda", dtype=dtype)
        need = raw.oq_matmul_nbits_workspace_bytes(M, K, N, 32, atype)
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
        st = raw.oq_matmul_nbits(c.x.data_ptr(), atype, M, K, K, c.blob.data_ptr(), 4, N, 32, c.scales.data_ptr(), 0, c.zero_points.data_ptr(),
                                 c.bias.data_ptr(), 0, y.data_ptr(), N + 5, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
        assert st == 0, raw.oq_last_error()
        assert torch.equal(y[:, :N], want) and (y[:, N:] == -77.0).all()


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_the_same_call_twice_gives_the_same_bytes(ops, dt):
    for M, K, N in ((70, 1024, 260), (3, 4096, 64)):                      # one pass over K, and K split across workgroups
        c = Case(gen(5), M, K, N, 128, 4, DTYPES[dt])
        first, second = c.run(ops), c.run(ops)
        assert torch.equal(first.view(torch.uint8), second.view(torch.uint8))


# ------------------------------------------------------------------------------------ 2. random data
RANDOM_SHAPES = [(70, 1024, 260, 128), (3, 4096, 64, 128)]


def rel_fro(y, y64):
    return ((y.to(torch.float64) - y64).norm() / y64.norm()).item()


@pytest.mark.parametrize("scales", ["fp32 scales", "scales of A's type"])
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=[str(s) for s in RANDOM_SHAPES])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_random_data_stays_inside_the_derived_bound_and_beside_the_expansion_route(ops, dt, bits, shape, scales):
    M, K, N, group = shape
    dtype = DTYPES[dt]
    c = Case(gen(21), M, K, N, group, bits, dtype, scale_dtype=torch.float32 if scales == "fp32 scales" else dtype)
    y, y64 = c.run(ops), c.y64()
    assert y.dtype == dtype and y.shape == (M, N)
    excess = ((y.to(torch.float64) - y64).abs() - c.bound()).max().item()
    ours, parents = rel_fro(y, y64), rel_fro(c.parent(), y64)
    print(f"{dt} bits={bits} {shape} {scales}: max(|err| - bound) = {excess:.3e}, rel. Frobenius {ours:.3e} (expansion route {parents:.3e})")
    assert excess <= 0.0
    assert ours <= 1.5 * parents


@pytest.mark.parametrize("factor", [1e30, 1e-30])
def test_fp32_rows_of_any_magnitude_keep_the_relative_bound(ops, factor):
    c = Case(gen(31), 70, 1024, 260, 128, 4, torch.float32, bias=False)
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
    c = Case(gen(41), M, K, N, 128, 4, DTYPES[dt])
    clean = c.run(ops)
    x = c.x.clone()
    x[2, K - 3] = float("nan")
    y = c.run(ops, x)
    assert torch.isnan(y[2]).all()
    keep = [m for m in range(M) if m != 2]
    assert torch.equal(y[keep], clean[keep])


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_a_zero_input_gives_exactly_the_bias(ops, dt):
    c = Case(gen(43), 19, 320, 45, 64, 8, DTYPES[dt])
    y = c.run(ops, torch.zeros_like(c.x))
    assert torch.equal(y, c.bias.expand(19, 45))


# ------------------------------------------------------------------------------------ 4. no expanded weight
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_no_expanded_weight_is_ever_allocated(ops, dt):
    M, K, N = 16, 1024, 1024
    c = Case(gen(51), M, K, N, 128, 4, DTYPES[dt])

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
    print(f"{dt}: peak growth fused {fused} B, expansion route {expanded} B, fp16 weight {N * K * 2} B")
    assert fused < N * K * 2
    assert expanded > N * K * 2                                            # the route it replaces does pay it: the test is not vacuous


# ------------------------------------------------------------------------------------ 5. refusals
def test_refusals_leave_y_untouched_and_the_op_raises_by_name(ops, lib):
    c = Case(gen(61), 8, 64, 16, 32, 4, torch.float16, integer=True)
    raw = lib.load()
    y = torch.full((8, 16), -77.0, device="cuda", dtype=torch.float16)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")

    def call(bits=4, group=32, flags=0, atype=1):
        return raw.oq_matmul_nbits(c.x.data_ptr(), atype, 8, 64, 64, c.blob.data_ptr(), bits, 16, group, c.scales.data_ptr(), 0,
                                   c.zero_points.data_ptr(), None, flags, y.data_ptr(), 16, ws.data_ptr(), ws.numel(),
                                   torch.cuda.current_stream().cuda_stream)

    for kw, status, word in ((dict(bits=2), -2, "bits"), (dict(group=16), -2, "group_size"), (dict(group=48), -2, "group_size"),
                             (dict(flags=1), -2, "float zero points"), (dict(flags=2), -2, "g_idx"), (dict(atype=5), -1, "atype")):
        assert call(**kw) == status
        assert word in raw.oq_last_error().decode()
    torch.cuda.synchronize()
    assert (y == -77.0).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(y, c.rounded(c.y64() - c.bias.to(torch.float64)))

    args = dict(K=64, N=16, bits=4, block_size=32)
    with pytest.raises(NotImplementedError, match="float zero points"):
        ops.matmul_nbits(c.x, c.blob, c.scales, torch.zeros(16, 2, device="cuda"), **args)
    with pytest.raises(NotImplementedError, match="block_size = 16"):
        ops.matmul_nbits(c.x, c.blob, c.scales, None, **{**args, "block_size": 16})
    with pytest.raises(NotImplementedError, match="bits = 2"):
        ops.matmul_nbits(c.x, c.blob, c.scales, None, **{**args, "bits": 2})
    with pytest.raises(NotImplementedError, match="float64"):
        ops.matmul_nbits(c.x.double(), c.blob, c.scales, None, **args)


def test_leading_axes_are_flattened_and_restored(ops):
    c = Case(gen(71), 24, 96, 40, 32, 4, torch.float16, integer=True)
    y = ops.matmul_nbits(c.x.reshape(2, 3, 4, 96), c.blob, c.scales, c.zero_points, K=96, N=40, bits=4, block_size=32, bias=c.bias)
    assert y.shape == (2, 3, 4, 40) and torch.equal(y.reshape(24, 40), c.rounded(c.y64()))
