"""The Hessian of fp32 activations (oq_hessian_accumulate_f32 and what sits on it: the prepared pair, the grouped chain;
csrc/gemm_tn.hip, csrc/syrk_bf16x3.hip) against `hessian_cases.expected`, bit for bit, under all four methods.

Every call goes through the C entry points with device pointers, so that n_seen, n_add, ldx, the base pointers and the workspace
size are free.  H lies between sentinel floats; on a first call it holds NaN (beta = 0 must not read it); every workspace is
filled with 0xFF bytes (pad rows, pad columns and slabs have to be written, not assumed zero); the gaps of a strided X hold 1e30.
n_total is 2, 8 or 32: 2 / n and sqrt(2 / n) are powers of two.

What is compared how.  `hessian_cases.exact_ok(...).mask` says where the result is an fp32 number that no summation order can
change: there the bits must be `expected`'s (a zero is +0.0: hessian_cases' docstring says why, nothing is mapped here).  The mask
is everything for bf16x6 and f16x3, and for every method on small integers and on `mid_pairs` (the recipe that holds the middle
products of bf16x9 to bits); under f32 and bf16x9, which keep every product, the
diagonal of a column with a three-piece element is no fp32 number, and those few elements are held to `summation_bound` instead
(test_hessian_cases.py counts them).  got == got.T always.  A failure prints `describe`: tile, wave, triangle and store arm.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hessian_cases as hc

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
PAD = 64                                  # sentinel floats on either side of H: 256 bytes, so H keeps torch's alignment


@pytest.fixture(scope="module")
def lib():
    from onnx_quantize_amd.hip import _lib
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(lib, status):
    assert status == 0, (status, lib.oq_last_error().decode())


@functools.lru_cache(maxsize=None)
def data(recipe, T, K):
    x = hc.RECIPES[recipe](T, K)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(method, recipe, T, K, n_seen, n_add):
    """Computed once per case and shared: (expected, the exact mask, kept sum, h0)."""
    x = data(recipe, T, K)
    h0 = hc.integer_h0(x, K) if n_seen else None
    ex = hc.exact_ok(method, x, n_seen, n_add, h0)
    assert ex.all or method in hc.KEEPS_EVERYTHING, (method, recipe, T, K)
    return hc.expected(method, x, n_seen, n_add, h0), ex.mask, h0


class Out:
    """H [K, K] inside a larger buffer, PAD sentinels before and after; `off` floats (0 or 1) move it off 16-byte alignment."""

    def __init__(self, K, h0=None, off=0):
        self.K, self.begin = K, PAD + off
        self.buf = torch.full((K * K + 2 * PAD + 4,), SENTINEL, dtype=torch.float32, device="cuda")
        h = self.buf[self.begin:self.begin + K * K]
        if h0 is None:
            h.fill_(float("nan"))
        else:
            h.copy_(torch.from_numpy(np.ascontiguousarray(h0, dtype=np.float32)).reshape(-1))
        self.ptr = self.buf.data_ptr() + 4 * self.begin
        assert (self.ptr % 16 == 0) == (off == 0)

    def result(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        end = self.begin + self.K * self.K
        assert (b[:self.begin] == SENTINEL).all() and (b[end:] == SENTINEL).all(), "a sentinel next to H was overwritten"
        return b[self.begin:end].reshape(self.K, self.K).copy()


def device_x(x, ldx=None, off=0):
    """x on the device with leading dimension ldx, `off` floats behind a 16-byte boundary; everything around it is 1e30."""
    T, K = x.shape
    ldx = K if ldx is None else ldx
    buf = torch.full((T * ldx + 8,), 1e30, dtype=torch.float32, device="cuda")
    view = buf[off:off + T * ldx].reshape(T, ldx)
    view[:, :K] = torch.from_numpy(np.array(x, dtype=np.float32))
    assert (view.data_ptr() % 16 == 0) == (off == 0)
    return buf, view.data_ptr()


def workspace(nbytes, off=0):
    raw = torch.full((nbytes + off + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    return raw, raw.data_ptr() + off


def full_workspace_bytes(lib, method, T, K):
    need = lib.oq_hessian_workspace_bytes(T, K)
    assert need >= hc.pieces_workspace_bytes(T, K) and lib.oq_hessian_pieces_bytes(T, K) == hc.pieces_workspace_bytes(T, K)
    return need


def accumulate(lib, method, x, n_seen=0, n_add=2, h0=None, ldx=None, x_off=0, h_off=0, ws_bytes=None):
    """One oq_hessian_accumulate_f32 call.  ws_bytes: None = what oq_hessian_workspace_bytes asks for, 0 = no workspace."""
    T, K = x.shape
    keep, xp = device_x(x, ldx, x_off)
    out = Out(K, h0 if n_seen else None, h_off)
    nbytes = full_workspace_bytes(lib, method, T, K) if ws_bytes is None else ws_bytes
    raw, wp = workspace(nbytes) if nbytes else (None, None)
    ok(lib, lib.oq_hessian_accumulate_f32(C.c_void_p(xp), T, K, K if ldx is None else ldx, n_seen, n_add, C.c_void_p(out.ptr), hc.METHOD_CODE[method],
                                          C.c_void_p(wp), nbytes, stream()))
    got = out.result()
    del keep, raw
    return got


def assert_matches(got, method, recipe, T, K, n_seen=0, n_add=2, slices=1, aligned=True, what=""):
    want, mask, h0 = reference(method, recipe, T, K, n_seen, n_add)
    wrong = (got.view(np.uint32) != want.view(np.uint32)) & mask
    what = f"{what} {method} {recipe} T={T} K={K} n={n_seen}+{n_add} slices={slices}"
    if wrong.any():
        text = hc.describe(wrong, method, K, sliced=slices > 1, aligned=aligned)
        i, j = np.argwhere(wrong)[0]
        text += f"; first at ({i}, {j}): got {got[i, j]!r}, want {want[i, j]!r}"
        print(f"{what}: {text}")
        raise AssertionError(f"{what}: {text}")
    if not mask.all():
        x = data(recipe, T, K)
        bound = hc.summation_bound(method, x, n_seen, n_add, slices, h0)
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        over = ~mask & ~(err <= bound)
        assert not over.any(), f"{what}: beyond the summation bound where no fp32 number holds the sum: {hc.describe(over, method, K, slices > 1, aligned)}"
    np.testing.assert_array_equal(got, got.T, err_msg=what)


recipes_of = hc.recipes_of


def slab_bytes_full(lib, method, T, K):
    return hc.slab_bytes_in(method, T, K, full_workspace_bytes(lib, method, T, K))


# ------------------------------------------------------------------------------------ 1. the contraction and the width
@pytest.mark.parametrize("which", (0, 1, 2), ids=("small_integers", "widest", "mid_pairs"))
@pytest.mark.parametrize("T", hc.CONTRACTION_T)
@pytest.mark.parametrize("method", hc.METHODS)
def test_every_edge_of_the_contraction(lib, method, T, which):
    """Less than an 8-row chunk, the 16-row bf16 stage, the 32-row fp16 stage and fp32 kBT; one to four (five for bf16) stages
    against rings of three and two: a slice shorter than the ring re-reads its last stage, and both `phase` copies of every stage
    loop run in every block (waves 0-3 and 4-7)."""
    recipe = recipes_of(method)[which]
    assert_matches(accumulate(lib, method, data(recipe, T, 40)), method, recipe, T, 40)


@pytest.mark.parametrize("which", (0, 1, 2), ids=("small_integers", "widest", "mid_pairs"))
@pytest.mark.parametrize("K", hc.WIDTH_K)
@pytest.mark.parametrize("method", hc.METHODS)
def test_every_edge_of_the_width(lib, method, K, which):
    """One column; the 128 and 256 tiles full, one short and one over; K % 4 != 0 (`vec_ok` false) and a last group of four that
    ends outside K (`full` false) in syrk_tile_store; 1, 3 and 6 (f32: up to 15) tiles, grids that are no multiple of 8 for
    xcd_remap."""
    recipe = recipes_of(method)[which]
    assert_matches(accumulate(lib, method, data(recipe, 33, K)), method, recipe, 33, K)


@pytest.mark.parametrize("which", (0, 1, 2), ids=("small_integers", "widest", "mid_pairs"))
@pytest.mark.parametrize("method", hc.METHODS)
def test_nine_tile_columns(lib, method, which):
    """The first tile row of upper_tile_of that leaves an 8 x 8 super-tile: 45 tiles, super-tiles (0, 0), (0, 1) and (1, 1)."""
    recipe, K = recipes_of(method)[which], hc.NINE_COLUMNS[method]
    assert hc.ceil_div(K, hc.TILE[method]) == 9
    assert_matches(accumulate(lib, method, data(recipe, 40, K)), method, recipe, 40, K)


# ------------------------------------------------------------------------------------ 2. operand forms
@pytest.mark.parametrize("which", (0, 1, 2), ids=("small_integers", "widest", "mid_pairs"))
@pytest.mark.parametrize("x_off", (0, 1), ids=("aligned", "plus4bytes"))
@pytest.mark.parametrize("extra", (0, 1, 4))
@pytest.mark.parametrize("method", hc.METHODS)
def test_operand_forms(lib, method, extra, x_off, which):
    """ldx = K, K + 1, K + 4 and a base 4 bytes behind a 16-byte boundary: only (ldx % 4 == 0, aligned) takes the VEC arm of
    gemm_tn_kernel's loads; the split kernels read 4 bytes at a time everywhere.  The gap behind a row holds 1e30."""
    T, K = hc.FORMS_SHAPE
    recipe = recipes_of(method)[which]
    assert_matches(accumulate(lib, method, data(recipe, T, K), ldx=K + extra, x_off=x_off), method, recipe, T, K, what=f"ldx K+{extra} off {x_off}")


@pytest.mark.parametrize("method", hc.METHODS)
def test_h_off_its_16_byte_alignment(lib, method):
    """H 4 bytes behind a 16-byte boundary: `vec_ok` of syrk_tile_store is false although K % 4 == 0."""
    T, K = hc.FORMS_SHAPE
    for ns, na in ((0, 2), (6, 2)):
        x = data("small_integers", T, K)
        got = accumulate(lib, method, x, ns, na, hc.integer_h0(x, K) if ns else None, h_off=1)
        assert_matches(got, method, "small_integers", T, K, ns, na, aligned=False)


# ------------------------------------------------------------------------------------ 3. T-slices
SLICE_CASES = [(m, T, K) for m in hc.METHODS for (T, K) in hc.SLICE_SHAPES[m]]


@pytest.mark.parametrize("which", (0, 1, 2), ids=("small_integers", "widest", "mid_pairs"))
@pytest.mark.parametrize("method,T,K", SLICE_CASES, ids=[f"{m}-{T}x{K}" for m, T, K in SLICE_CASES])
def test_t_slices(lib, method, T, K, which):
    """1, 2 and >= 3 slices with a ragged last one (test_hessian_cases.py proves the counts), then the same call with (a) no
    room for slabs -- the pieces only; for f32 no workspace at all -- and (b) room for exactly two slabs: on exact data the bits
    do not depend on the slicing."""
    recipe = recipes_of(method)[which]
    x = data(recipe, T, K)
    count = hc.slices_of(method, T, K, slab_bytes_full(lib, method, T, K)).count
    assert count == hc.SLICE_SHAPES[method][(T, K)]
    first = accumulate(lib, method, x)
    assert_matches(first, method, recipe, T, K, slices=count, what="full workspace")
    none = 0 if method == "f32" else hc.pieces_workspace_bytes(T, K)
    two = 2 * K * K * 4 if method == "f32" else hc.pieces_workspace_bytes(T, K, 2 * K * K * 4)
    for label, nbytes in (("no slabs", none), ("two slabs", two)):
        n = hc.slices_of(method, T, K, hc.slab_bytes_in(method, T, K, nbytes)).count
        assert n <= 2
        got = accumulate(lib, method, x, ws_bytes=nbytes)
        assert_matches(got, method, recipe, T, K, slices=n, what=label)


# ------------------------------------------------------------------------------------ 4. the running average
RUNNING = [(m, T, K) for m in hc.METHODS for (T, K) in hc.RUNNING_SHAPES[m]]


@pytest.mark.parametrize("which", (0, 1, 2), ids=("small_integers", "widest", "mid_pairs"))
@pytest.mark.parametrize("n_seen,n_add", hc.N_TOTALS)
@pytest.mark.parametrize("method,T,K", RUNNING, ids=[f"{m}-{T}x{K}" for m, T, K in RUNNING])
def test_running_average(lib, method, T, K, n_seen, n_add, which):
    """beta = 0 (H holds NaN), 1/2, 3/4, 1/2 with alpha 1, 1, 1/4, 1/16 on an integer H: the direct epilogue with the vector
    (K = 260) and the scalar (K = 257) arm, and the reduction of a sliced call."""
    recipe = recipes_of(method)[which]
    x = data(recipe, T, K)
    count = hc.slices_of(method, T, K, slab_bytes_full(lib, method, T, K)).count
    assert (count > 1) == (T > 33)
    got = accumulate(lib, method, x, n_seen, n_add, hc.integer_h0(x, K) if n_seen else None)
    assert_matches(got, method, recipe, T, K, n_seen, n_add, slices=count)


# ------------------------------------------------------------------------------------ 5. the fp16 scale and the guard
@pytest.mark.parametrize("recipe", ["scaled(-50)", "scaled(0)", "scaled(50)", "guarded", "maximum_last"])
def test_f16x3_scale_and_guard(lib, recipe):
    """2^-50 reaches the clamp of the scale's exponent (60); the guarded column keeps one fp16 unit per live sample, the dead one and
    the column of -0.0 give +0.0; the maximum in the last row and column of 2081 rows sits behind the 2048-block absmax partition."""
    T, K = hc.SCALE_SHAPE
    x = data(recipe, T, K)
    if recipe == "scaled(-50)":
        assert hc.batch_scale(x) == 2.0 ** 60 and 15 - int(np.frexp(np.abs(x).max())[1]) > 60
    got = accumulate(lib, "f16x3", x)
    assert_matches(got, "f16x3", recipe, T, K, slices=hc.slices_of("f16x3", T, K, slab_bytes_full(lib, "f16x3", T, K)).count)
    if recipe == "guarded":
        assert got[1, 1] > 0 and got[2, 2] == 0 and not np.signbit(got[3]).any() and not got[3].any()


# ------------------------------------------------------------------------------------ 6. auto
def test_auto_takes_the_method_the_header_states(lib):
    """K = 2048 with the pieces' workspace: the bits of f16x3; K = 2047: those of f32; K = 2048 without a workspace: f32."""
    for (T, K), nbytes, method in (((8, 2048), None, "f16x3"), ((8, 2047), None, "f32"), ((8, 2048), 0, "f32")):
        want_f16, _, _ = reference("f16x3", "two_pieces_low", T, K, 0, 2)
        want_f32, _, _ = reference("f32", "two_pieces_low", T, K, 0, 2)
        assert (want_f16 != want_f32).any() and reference("f32", "two_pieces_low", T, K, 0, 2)[1].all()
        x = data("two_pieces_low", T, K)
        keep, xp = device_x(x)
        out = Out(K)
        nbytes = full_workspace_bytes(lib, method, T, K) if nbytes is None else nbytes
        raw, wp = workspace(nbytes) if nbytes else (None, None)
        ok(lib, lib.oq_hessian_accumulate_f32(C.c_void_p(xp), T, K, K, 0, 2, C.c_void_p(out.ptr), hc.METHOD_CODE["auto"], C.c_void_p(wp), nbytes, stream()))
        assert_matches(out.result(), method, "two_pieces_low", T, K, what=f"auto, {nbytes} bytes")


# ------------------------------------------------------------------------------------ 7. the prepared pair
def test_prepared_pair(lib):
    """prepare + accumulate_prepared = kept_sum('f16x3') at one tile, six tiles sliced and nine tile columns; the piece buffer is
    the same for all shapes, widest first (nothing stale is read); the slab buffer holds 0xFF and starts 4 bytes behind a 256-byte
    boundary."""
    shapes = sorted(hc.PREPARED_SHAPES, key=lambda s: -s[1])
    assert shapes[0][1] > shapes[-1][1]
    need = max(lib.oq_hessian_pieces_bytes(T, K) for T, K in shapes)
    raw, pieces = workspace(need + 256)
    pieces += (-pieces) % 256
    slab_raw = torch.full((3 * 520 * 520 * 4 + 1024,), 0xFF, dtype=torch.uint8, device="cuda")
    slabs = slab_raw.data_ptr() + (-slab_raw.data_ptr()) % 256 + 4
    slab_bytes = slab_raw.numel() - (slabs - slab_raw.data_ptr())
    for T, K in shapes:
        for recipe in ("small_integers", "two_pieces"):
            for ns, na in ((0, 2), (6, 2)):
                x = data(recipe, T, K)
                keep, xp = device_x(x)
                out = Out(K, hc.integer_h0(x, K) if ns else None)
                assert lib.oq_hessian_pieces_bytes(T, K) <= need
                ok(lib, lib.oq_hessian_prepare_f32(C.c_void_p(xp), T, K, K, ns + na, C.c_void_p(pieces), need, stream()))
                ok(lib, lib.oq_hessian_accumulate_prepared_f32(C.c_void_p(pieces), T, K, ns, na, C.c_void_p(out.ptr), C.c_void_p(slabs), slab_bytes, stream()))
                count = hc.slices_of("f16x3", T, K, (slab_bytes - 256) // 4 * 4).count
                assert (count > 1) == ((T, K) == (993, 520))
                assert_matches(out.result(), "f16x3", recipe, T, K, ns, na, slices=count, what="prepared")


# ------------------------------------------------------------------------------------ 8. the grouped chain
def grouped(lib, rows):
    """rows: (T, K, ldx, n_seen, n_add, recipe) -> the results of one oq_hessian_accumulate_many_f32 call, in that order."""
    keeps, outs, table = [], [], []
    for T, K, ldx, ns, na, recipe in rows:
        x = data(recipe, T, K)
        keep, xp = device_x(x, ldx)
        out = Out(K, hc.integer_h0(x, K) if ns else None)
        keeps.append(keep)
        outs.append(out)
        table.append((xp, out.ptr, T, K, ldx, ns, na, 0))
    assert len({r[1] for r in table}) == len(table)
    host = np.ascontiguousarray(np.array(table, dtype=np.int64))
    dev = torch.from_numpy(host).cuda()
    hp = C.c_void_p(host.ctypes.data)
    need = lib.oq_hessian_many_workspace_bytes(hp, len(table))
    assert need > 0
    raw, wp = workspace(need)
    ok(lib, lib.oq_hessian_accumulate_many_f32(hp, C.c_void_p(dev.data_ptr()), len(table), C.c_void_p(wp), need, stream()))
    return [o.result() for o in outs]


def test_grouped_chain(lib):
    """oq_hessian_accumulate_many_f32 called directly (the Python wrapper keeps small and ragged items away from it): one column;
    a ragged tile with ldx = K + 1; 513 rows with the maximum in the last one (256 absmax blocks of three rows); six tiles; one
    full tile; nine tile columns.  One table, the same table reversed, and every item alone: `split0` / `tile0` and
    `item_of_block` see every item first, last and in between."""
    rows = hc.grouped_table()
    assert [r[:2] for r in rows] == hc.GROUPED_ITEMS and any(r[2] == r[1] + 1 for r in rows) and len({r[3] for r in rows}) > 2
    for label, order in (("table", rows), ("reversed", rows[::-1])) + tuple((f"alone {i}", [r]) for i, r in enumerate(rows)):
        for (T, K, ldx, ns, na, recipe), got in zip(order, grouped(lib, order)):
            assert_matches(got, "f16x3", recipe, T, K, ns, na, what=f"grouped, {label}")


# ------------------------------------------------------------------------------------ 9. any data: every element against its own bound
TOLERANCE = [(m, T, K) for m in hc.METHODS for (T, K) in hc.TOLERANCE_SHAPES[m]]


@pytest.mark.parametrize("recipe", ["normal", "outlier_channels"])
@pytest.mark.parametrize("method,T,K", TOLERANCE, ids=[f"{m}-{T}x{K}" for m, T, K in TOLERANCE])
def test_every_element_within_its_summation_bound(lib, method, T, K, recipe):
    """|got - expected| <= (products * padded_rows + slices + 3) 2^-24 sum |a| |b| per ELEMENT (hessian_cases.summation_bound: one
    rounding per accumulated product, per slice addition and for the epilogue), not against max |H|: a wrong element between two
    small channels -- the outlier channels are 1e5 apart -- is far outside.  The largest ratio is printed."""
    x = data(recipe, T, K)
    h0 = hc.integer_h0(x, K)
    count = hc.slices_of(method, T, K, slab_bytes_full(lib, method, T, K)).count
    for ns, na in ((0, 2), (6, 2)):
        got = accumulate(lib, method, x, ns, na, h0 if ns else None)
        want = hc.expected(method, x, ns, na, h0 if ns else None).astype(np.float64)
        bound = hc.summation_bound(method, x, ns, na, count, h0 if ns else None)
        err = np.abs(got.astype(np.float64) - want)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
        print(f"{method} {recipe} T={T} K={K} n={ns}+{na} slices={count}: max |got - expected| / bound = {ratio.max():.4f}")
        over = ratio > 1
        assert not over.any(), f"{method} {recipe} T={T} K={K}: {hc.describe(over, method, K, count > 1)}; worst ratio {ratio.max():.3f}"
        np.testing.assert_array_equal(got, got.T)
        if recipe == "outlier_channels" and ns == 0:       # afterwards a dead channel holds beta h0
            assert not got[7].any() and not got[:, 7].any()
