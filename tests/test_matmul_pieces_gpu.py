"""The fp16-piece GEMM behind oq_matmul_pieces_bytes / oq_matmul_prepare_f32 / oq_matmul_pieces_f32 (include/oq_hip.h, N1;
csrc/syrk_bf16x3.hip: gemm_f16x3_body, f16_m16_mainloop, staged_tile_epilogue and the preparation kernels), called through the C
entry points with device pointers so that every call form is reached, not only the one `ops.matmul_pieces` makes.

1  exact integers (piece_gemm_cases.py: recipes that satisfy `exact_ok`, checked on the CPU in test_piece_gemm_cases.py): the
   result is torch.equal to the float64 product rounded to fp32 -- at every tile, contraction, operand, store and alpha / beta
   form, and beyond 2048 source rows of the absmax partition.  A failure prints `describe`: the tile slots that are wrong.
   The tile grid and the contraction edges run twice: with `a_two_pieces`, and with `both_two_pieces`, under which lo . hi AND
   hi . lo are live in every slot (B of `a_two_pieces` has no lo piece: a wrong hi . lo would multiply zeros there).
2  buffers: guards around every piece buffer, a prepared weight is read-only, a product is reproducible.
3  magnitudes on random data against `emulate`, which holds the same pieces and the same three products: only the fp32
   summation separates the two, |got - emulate| <= (3 * 32 * ceil(Kd / 32) + 3) 2^-24 mass / (s_a s_b) (derived in
   piece_gemm_cases.py), Kd <= 512 so that this stays below a dropped piece's 2^-11.
4  containment of NaN / Inf and of zeros.   5  the `ops` wrappers.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import piece_gemm_cases as pg

pytestmark = pytest.mark.gpu
GUARD, PATTERN = 256, 0xA5
SENTINEL = -12345.0
A_FORMS = ("row", "operand", "kmajor")            # [M, Kd] with per-row scales, [M, Kd] with the operand's scale, [Kd, M]
B_FORMS = ("kmajor", "fast")                      # [Kd, N], [N, Kd]


@pytest.fixture(scope="module")
def lib():
    from onnx_quantize_amd.hip import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ops():
    from onnx_quantize_amd.hip import ops
    return ops


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(lib, status):
    assert status == 0, (status, lib.oq_last_error().decode())


class Pieces:
    """One operand's piece buffer: the `oq_matmul_pieces_bytes` window, 256-byte aligned, with at least GUARD bytes of PATTERN on both sides."""

    def __init__(self, lib, Kd, cols):
        self.need = lib.oq_matmul_pieces_bytes(Kd, cols)
        assert self.need >= pg.pieces_bytes_at_least(Kd, cols)
        self.raw = torch.full((self.need + 2 * GUARD + 256,), PATTERN, dtype=torch.uint8, device="cuda")
        self.off = GUARD + (-(self.raw.data_ptr() + GUARD)) % 256
        self.ptr = self.raw.data_ptr() + self.off
        assert self.ptr % 256 == 0 and self.raw.numel() - self.off - self.need >= GUARD

    def guards_intact(self):
        return bool((self.raw[:self.off] == PATTERN).all() and (self.raw[self.off + self.need:] == PATTERN).all())


def prepare(lib, src, Kd, cols, fast, per_row, extra=0):
    """src: numpy [cols, Kd] (fast) or [Kd, cols]; the source on the device has `extra` more floats per row than it needs, 1e30
    each: a stray read of the gap changes the scale and with it the bits."""
    rows, n = src.shape
    assert (rows, n) == ((cols, Kd) if fast else (Kd, cols))
    wide = torch.full((rows, n + extra), 1e30, dtype=torch.float32, device="cuda")
    wide[:, :n] = torch.from_numpy(np.ascontiguousarray(src, dtype=np.float32))
    p = Pieces(lib, Kd, cols)
    ok(lib, lib.oq_matmul_prepare_f32(C.c_void_p(wide.data_ptr()), Kd, cols, n + extra, fast, per_row, C.c_void_p(p.ptr), p.need, stream()))
    return p


def prepare_a(lib, a, form="row", extra=0):
    M, Kd = a.shape
    return prepare(lib, a.T, Kd, M, 0, 0, extra) if form == "kmajor" else prepare(lib, a, Kd, M, 1, int(form == "row"), extra)


def prepare_b(lib, b, form="kmajor", extra=0):
    Kd, N = b.shape
    return prepare(lib, b, Kd, N, 0, 0, extra) if form == "kmajor" else prepare(lib, b.T, Kd, N, 1, 0, extra)


def product(lib, pa, pb, M, N, Kd, per_row, alpha=1.0, beta=0.0, out=None, c_ptr=None, ldc=None):
    if out is None and c_ptr is None:
        out = torch.empty((M, N), dtype=torch.float32, device="cuda")
    ok(lib, lib.oq_matmul_pieces_f32(C.c_void_p(pa.ptr), C.c_void_p(pb.ptr), M, N, Kd, alpha, beta,
                                      C.c_void_p(out.data_ptr() if c_ptr is None else c_ptr), N if ldc is None else ldc, int(per_row), stream()))
    return out


def run(lib, a, b, a_form="row", b_form="kmajor", extra=0, **kw):
    (M, Kd), N = a.shape, b.shape[1]
    pa, pb = prepare_a(lib, a, a_form, extra), prepare_b(lib, b, b_form, extra)
    out = product(lib, pa, pb, M, N, Kd, a_form == "row", **kw)
    torch.cuda.synchronize()
    assert pa.guards_intact() and pb.guards_intact(), "a piece buffer's guard bytes were written"
    return out


def product64(a, b):
    want = a.astype(np.float64) @ b.astype(np.float64)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    return torch.from_numpy(want.astype(np.float32))


def assert_exact(got, want, what, ldc=None, aligned=True):
    got = got.cpu()
    if not torch.equal(got, want):
        text = pg.describe((got != want).numpy(), ldc=ldc, aligned=aligned)
        print(f"{what}: {text}")
        raise AssertionError(f"{what}: {text}")


# ------------------------------------------------------------------------------------ 1. exact integers
@pytest.mark.parametrize("recipe", pg.GRID_RECIPES)
@pytest.mark.parametrize("MN", pg.TILE_GRID, ids=[f"{M}x{N}" for M, N in pg.TILE_GRID])
def test_every_tile_of_the_grid(lib, MN, recipe):
    """One block, a row of blocks, a column of blocks, a 2 x 3 grid (a swapped tile_m / tile_n reads another tile's operands), tiles
    whose last rows / columns are padding."""
    M, N = MN
    a, b = pg.RECIPES[recipe](M, 100, N)
    assert_exact(run(lib, a, b), product64(a, b), f"{recipe} {M} x 100 x {N}")


@pytest.mark.parametrize("recipe", pg.GRID_RECIPES)
@pytest.mark.parametrize("Kd", pg.CONTRACTIONS)
def test_every_edge_of_the_contraction(lib, Kd, recipe):
    """Less than a chunk of 8 rows, less than a stage of 32, one to four stages (the ring of two with odd and even counts), a
    ragged last chunk, 32 stages."""
    a, b = pg.RECIPES[recipe](70, Kd, 37)
    assert_exact(run(lib, a, b), product64(a, b), f"{recipe} 70 x {Kd} x 37")


@pytest.mark.parametrize("recipe", sorted(pg.RECIPES))
def test_a_contraction_of_1000_with_every_recipe(lib, recipe):
    a, b = pg.RECIPES[recipe](70, 1000, 37)
    assert_exact(run(lib, a, b), product64(a, b), f"{recipe} 70 x 1000 x 37")


@pytest.mark.parametrize("extra", [0, 5], ids=["ldx at its minimum", "ldx 5 above"])
@pytest.mark.parametrize("b_form", B_FORMS)
@pytest.mark.parametrize("a_form", A_FORMS)
def test_every_operand_form(lib, a_form, b_form, extra):
    M, Kd, N = pg.FORMS_SHAPE
    for recipe in (pg.a_two_pieces, pg.b_two_pieces):
        a, b = recipe(M, Kd, N)
        assert_exact(run(lib, a, b, a_form, b_form, extra), product64(a, b), f"{recipe.__name__}, A {a_form}, B {b_form}, ldx + {extra}")


def store_case(lib, N, ldc, offset):
    """C at `offset` floats behind a 16-byte boundary inside a buffer of sentinels: the product is exact, and what lies in front
    of C, in the gap columns and behind the last row keeps its sentinel; with beta = 1 over zeros the same bits come back through
    the read-modify-write."""
    M, Kd = 70, 100
    a, b = pg.a_two_pieces(M, Kd, N)
    want = product64(a, b)
    pa, pb = prepare_a(lib, a), prepare_b(lib, b)
    for beta in (0.0, 1.0):
        flat = torch.full((8 + M * ldc + 8,), SENTINEL, dtype=torch.float32, device="cuda")
        assert flat.data_ptr() % 16 == 0
        start = 4 + offset
        window = flat[start:start + M * ldc].view(M, ldc)[:, :N]
        if beta != 0.0:
            window.zero_()
        product(lib, pa, pb, M, N, Kd, True, beta=beta, c_ptr=flat.data_ptr() + 4 * start, ldc=ldc)
        assert_exact(window.clone(), want, f"N {N}, ldc {ldc}, offset {offset}, beta {beta}", ldc=ldc, aligned=offset == 0)
        window.fill_(SENTINEL)
        assert bool((flat == SENTINEL).all()), f"N {N}, ldc {ldc}, offset {offset}, beta {beta}: written outside C [M, N]"
    assert pa.guards_intact() and pb.guards_intact()


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned base", "base one float off"])
@pytest.mark.parametrize("ldc_extra", [0, 1, 4])
@pytest.mark.parametrize("N", pg.STORE_N)
def test_every_store_form(lib, N, ldc_extra, offset):
    """Vector stores (ldc % 4 == 0 and a 16-byte aligned base), the scalar path otherwise and in a row's last partial group of
    four."""
    store_case(lib, N, N + ldc_extra, offset)


@pytest.mark.parametrize("ldc", [40, 44])
@pytest.mark.parametrize("N", [37, 38, 39])
def test_vector_rows_that_end_in_a_partial_group(lib, N, ldc):
    """ldc % 4 == 0 and an aligned base with N % 4 != 0: every row is vectors and then one to three scalars (`col + 3 < N`); a
    vector there would write the gap -- or, with ldc = N + 1, the next row's first column."""
    store_case(lib, N, ldc, 0)


@pytest.mark.parametrize("N", [36, 37], ids=["vector stores", "scalar stores"])
def test_beta_zero_does_not_read_c(lib, N):
    a, b = pg.a_two_pieces(70, 100, N)
    out = torch.full((70, N), float("nan"), dtype=torch.float32, device="cuda")
    pa, pb = prepare_a(lib, a), prepare_b(lib, b)
    product(lib, pa, pb, 70, N, 100, True, beta=0.0, out=out)
    assert not out.isnan().any()
    assert_exact(out, product64(a, b), f"beta = 0 over NaN, N {N}", ldc=N)


@pytest.mark.parametrize("N", [36, 37], ids=["vector stores", "scalar stores"])
def test_alpha_and_beta(lib, N):
    a, b = pg.a_two_pieces(70, 100, N)
    c = pg.integer_c(70, N)
    pa, pb = prepare_a(lib, a), prepare_b(lib, b)
    for alpha, beta in itertools.product((1.0, -1.0, 0.25, 3.0), (1.0, 0.5, -2.0)):
        assert pg.epilogue_ok(a, b, True, alpha, beta, c)
        want = beta * c.astype(np.float64) + alpha * (a.astype(np.float64) @ b.astype(np.float64))
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
        out = torch.from_numpy(c).cuda()
        product(lib, pa, pb, 70, N, 100, True, alpha=alpha, beta=beta, out=out)
        assert_exact(out, torch.from_numpy(want.astype(np.float32)), f"alpha {alpha}, beta {beta}, N {N}", ldc=N)


def test_two_accumulating_calls_equal_one(lib):
    """Kd = 40 + 60 with beta = 1 on the second call against Kd = 100 in one: the same bytes."""
    M, Kd, N = pg.FORMS_SHAPE
    a, b = pg.a_two_pieces(M, Kd, N)
    one = run(lib, a, b)
    two = run(lib, a[:, :40], b[:40])
    pa, pb = prepare_a(lib, a[:, 40:]), prepare_b(lib, b[40:])
    product(lib, pa, pb, M, N, 60, True, beta=1.0, out=two)
    assert_exact(two, one.cpu(), "40 + 60 against 100")
    assert_exact(one, product64(a, b), "Kd = 100 in one call")


@pytest.mark.parametrize("which", ["b", "a"], ids=["k-major B of 2081 rows", "fast-axis A of 2081 rows, operand scale"])
def test_the_absmax_partition_beyond_2048_rows(lib, which):
    """The single largest element sits in the last source row: a maximum taken over the first 2048 rows only gives a scale under
    which that element overflows fp16."""
    a, b, per_row = pg.beyond_2048_rows(which)
    assert_exact(run(lib, a, b, "row" if per_row else "operand"), product64(a, b), f"{a.shape[0]} x {a.shape[1]} x {b.shape[1]}")


# ------------------------------------------------------------------------------------ 2. buffers
@pytest.mark.parametrize("shape", pg.GUARD_SHAPES, ids=["x".join(map(str, s)) for s in pg.GUARD_SHAPES])
def test_guards_around_the_piece_buffers_survive(lib, shape):
    """`run` checks the guard bytes on both sides of both windows behind prepare and product: all three A forms, both B forms."""
    a, b = pg.a_two_pieces(*shape)
    want = product64(a, b)
    for a_form, b_form in itertools.product(A_FORMS, B_FORMS):
        assert_exact(run(lib, a, b, a_form, b_form), want, f"{shape}, A {a_form}, B {b_form}")


def test_a_prepared_weight_is_read_only(lib):
    M, Kd, N = pg.FORMS_SHAPE
    a, b = pg.a_two_pieces(M, Kd, N)
    pb = prepare_b(lib, b)
    torch.cuda.synchronize()
    before = pb.raw.clone()
    for x in (a, -a, a[::-1]):
        pa = prepare_a(lib, x)
        assert_exact(product(lib, pa, pb, M, N, Kd, True), product64(x, b), "a prepared weight against three A")
    assert torch.equal(pb.raw, before)


def test_the_same_product_twice_gives_the_same_bytes(lib):
    a, b = pg.magnitude_case("plain", (260, 512, 40))
    first, second = run(lib, a, b), run(lib, a, b)
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    pa, pb = prepare_a(lib, a), prepare_b(lib, b)
    outs = [product(lib, pa, pb, 260, 40, 512, True) for _ in range(3)]
    assert all(torch.equal(o.view(torch.int32), first.view(torch.int32)) for o in outs)


# ------------------------------------------------------------------------------------ 3. magnitudes
@pytest.mark.parametrize("case", pg.magnitude_cases(), ids=[f"{kind}-{'x'.join(map(str, shape))}-{'row' if per_row else 'operand'}"
                                                            for kind, shape, per_row in pg.magnitude_cases()])
def test_magnitudes_against_the_emulation(lib, case):
    kind, shape, per_row = case
    a, b = pg.magnitude_case(kind, shape)
    em = pg.emulate(a, b, per_row)
    bound = pg.summation_bound(em, shape[1])
    got = run(lib, a, b, "row" if per_row else "operand").cpu().numpy().astype(np.float64)
    err = np.abs(got - em.y)
    live = bound > 0
    print(f"{kind} {shape} per_row={per_row}: max |got - emulate| / bound = {(err[live] / bound[live]).max():.4f}")
    bad = ~(err <= bound)                                              # a NaN is bad
    assert not bad.any(), pg.describe(bad)


# ------------------------------------------------------------------------------------ 4. containment
@pytest.mark.parametrize("poison", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_element_stays_in_its_row_under_per_row_scales(lib, poison):
    """A NaN or an Inf in row r of A: that row's scale is 1, its hi piece is the NaN / Inf and (for an Inf) its lo piece Inf - Inf,
    so every element of output row r is non-finite, whatever B holds there; every other row keeps the bytes of the run without it."""
    M, Kd, N = pg.FORMS_SHAPE
    a, b = pg.one_piece(M, Kd, N)
    clean = run(lib, a, b)
    assert_exact(clean, product64(a, b), "the clean run")
    for r, k in ((5, 17), (69, 99), (0, 0)):
        x = a.copy()
        x[r, k] = poison
        got = run(lib, x, b)
        assert not torch.isfinite(got[r]).any(), (r, k)
        keep = [i for i in range(M) if i != r]
        assert torch.equal(got[keep].view(torch.int32), clean[keep].view(torch.int32)), (r, k)


@pytest.mark.parametrize("a_form", ["operand", "kmajor"])
@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_a_non_finite_element_under_the_operand_scale(lib, poison, a_form):
    """The operand's maximum is non-finite, so its scale falls to 1 and every element is split as it is: the poisoned row is
    non-finite throughout, and the other rows are what hi = fp16(x), lo = fp16(x - hi) give -- exact for `one_piece`, whose integers
    fp16 holds -- where a finite operand of this size would have been scaled up first.  (Elements beyond fp16's range would
    overflow under that scale: the per-row form is the one that contains a non-finite row.)"""
    M, Kd, N = pg.FORMS_SHAPE
    a, b = pg.one_piece(M, Kd, N)
    want = product64(a, b)
    x = a.copy()
    x[5, 17] = poison
    assert pg.split(x, False)[2].item() == 1.0
    got = run(lib, x, b, a_form).cpu()
    assert not torch.isfinite(got[5]).any()
    keep = [i for i in range(M) if i != 5]
    assert_exact(got[keep], want[keep], f"rows beside the poisoned one, A {a_form}")


def test_zero_rows_and_zero_operands_give_exact_zeros(lib):
    M, Kd, N = pg.FORMS_SHAPE
    a, b = pg.one_piece(M, Kd, N)
    x = a.copy()
    x[5] = 0.0
    x[69] = 0.0
    for a_form in A_FORMS:
        got = run(lib, x, b, a_form)
        assert bool((got[5] == 0).all() and (got[69] == 0).all())
        assert_exact(got, product64(x, b), f"two zero rows, A {a_form}")
        assert bool((run(lib, np.zeros_like(a), b, a_form) == 0).all())
        for b_form in B_FORMS:
            assert bool((run(lib, a, np.zeros_like(b), a_form, b_form) == 0).all())


# ------------------------------------------------------------------------------------ 5. the wrappers
def test_the_wrapper_takes_views_and_refuses_mismatches(ops):
    M, Kd, N = pg.FORMS_SHAPE
    a, b = pg.a_two_pieces(M, Kd, N)
    x = torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()                       # [M, Kd] with the rows on the fast axis
    wide = torch.full((Kd, N + 13), 1e30, dtype=torch.float32, device="cuda")
    wide[:, :N] = torch.from_numpy(b)
    w = wide[:, :N]                                                                   # a column slice: rows 13 floats apart
    assert not x.is_contiguous() and not w.is_contiguous()
    want = ops.matmul_pieces(x.contiguous(), w.contiguous())
    assert_exact(want, product64(a, b), "ops.matmul_pieces on contiguous operands")
    for xs, ws in ((x, w), (x, w.contiguous()), (x.contiguous(), w), (x.contiguous().reshape(7, 10, Kd), w)):
        got = ops.matmul_pieces(xs, ws)
        assert got.shape == (*xs.shape[:-1], N) and torch.equal(got.reshape(M, N).view(torch.int32), want.view(torch.int32))
    prepared = ops.matmul_prepare(w, False)
    assert torch.equal(ops.matmul_pieces(x, prepared).view(torch.int32), want.view(torch.int32))
    with pytest.raises(ValueError):
        ops.matmul_pieces(x[:, :Kd - 1], w)                                           # contraction mismatch
    with pytest.raises(ValueError):
        ops.matmul_pieces(x, prepared.__class__(prepared.pieces, Kd + 1, N))
    with pytest.raises(ValueError):
        ops.matmul_pieces(x, torch.zeros((2, Kd, N), device="cuda"))                  # a 3-d weight
