"""The AWQ / SmoothQuant searches (csrc/awq.hip) at the edges of each route, against the oracle.

A candidate's residual D = W - W^ comes from awq_group_diff_kernel (fused, with or without pieces output), awq_diff4_kernel or
awq_diff_kernel; its loss from the direct product X D, the Gram form <D, G D>, or the Gram form from streamed statistics.  The
route follows from N % 4, ldw % 4, the alignment of W, g, K % 32, T >= 3 K and the entry point.  The whole-matrix tests of
tests/test_preprocessing.py run i.i.d. inputs through these routes, where a wrong last column tile, a dropped tail row or a
misplaced row scale moves the total by less than the bar; the cases here put the loss where such a mistake would be
(tests/awq_cases.py, whose conditions tests/test_awq_cases.py checks on the CPU and section 1 checks again before comparing).

Bars:
* losses, rtol 2e-3: twice the worst case of the loss product's 11-bit first pieces (2 * 2^-11 = 9.8e-4; D enters the product
  rounded to 11 bits and the loss is quadratic in it).  The chosen point's oracle loss is at most min * (1 + 2e-3).
* the winner's scale and every candidate's scale, rtol 1e-5: the project's existing bar for the search scale (reductions in another
  order, powf against np.power: a few ulp).
* SmoothQuant scale, rtol 2e-6: the project's existing bar (tests/test_preprocessing.py).
* strided against contiguous operands on one route, workspace in a guarded buffer against the `ops` call: equal bits -- the same
  kernels doing the same arithmetic in the same order.

Sections (each test's docstring names the kernels and routes it reaches):
  1  spotlight cases on the array, Gram and statistics routes        4  a dead channel next to an outlier channel
  2  every candidate's scale, `best_out`, host-side refusals         5  SmoothQuant shapes, strides, alpha, zero rows
  3  small and odd shapes, both sides of T = 3 K, strided operands   6  the searches stay inside the workspace they ask for
Every figure is printed before it is asserted (`AWQ-EDGE section ... deviation ...`)."""
import ctypes as C

import numpy as np
import pytest

import awq_cases as A
import oq_oracle as O

pytestmark = pytest.mark.gpu

LOSS_RTOL, SCALE_RTOL, SQ_RTOL = 2e-3, 1e-5, 2e-6
MIB = 1 << 20


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()            # a copy: the shared cases are read-only


def _statistics(xd):
    """`ops.SearchStatistics` of xd [T, K] fed in two uneven batches (one row alone when there are fewer than six)."""
    from onnx_quantize_amd.hip import ops
    st = ops.SearchStatistics(xd.shape[1], "cuda")
    cut = 5 if xd.shape[0] > 5 else 1
    st.add(xd[:cut])
    st.add(xd[cut:])
    assert st.rows == xd.shape[0]
    return st


def _searches(route, x, w, qtype, strategy, g, sym=False, reduce_range=False):
    """Both searches through `ops` on one route: (winning scale, losses[20], clip ratio, losses[10])."""
    from onnx_quantize_amd.hip import ops
    wd = _dev(w)
    if route == "stats":
        st = _statistics(_dev(x))
        s, l = ops.awq_scale_search_stats(st, wd, qtype, strategy, g, sym, reduce_range)
        r, cl = ops.awq_clip_search_stats(st, wd, qtype, strategy, g, sym, reduce_range)
    else:
        xd = _dev(A.tiled_for_gram(x, x.shape[1]) if route == "gram" else x)
        assert (xd.shape[0] >= 3 * xd.shape[1]) == (route == "gram"), (route, tuple(xd.shape))      # the route the case is meant for
        s, l = ops.awq_scale_search(xd, wd, qtype, strategy, g, sym, reduce_range)
        r, cl = ops.awq_clip_search(xd, wd, qtype, strategy, g, sym, reduce_range)
    return s.cpu().numpy(), l, r, cl


def _deviation(l, el):
    return float(np.max(np.abs(np.asarray(l, np.float64) / np.asarray(el, np.float64) - 1.0)))


def _compare(section, tag, got, want):
    """The bars of tests/test_preprocessing.py on both searches; the figures first."""
    (s, l, r, cl), (es, el, er, ecl) = got, want
    same = int(np.argmin(l)) == int(np.argmin(el))
    sdev = float(np.max(np.abs(s / es - 1.0))) if same else float("nan")
    print(f"AWQ-EDGE section {section} {tag}: scale-search deviation {_deviation(l, el):.3e}, clip-search deviation {_deviation(cl, ecl):.3e}, "
          f"winner {int(np.argmin(l))} (oracle {int(np.argmin(el))}), winner's scale deviation {sdev:.3e}, clip ratio {r} (oracle {er})")
    np.testing.assert_allclose(l, el, rtol=LOSS_RTOL, err_msg=tag)
    assert el[int(np.argmin(l))] <= el.min() * (1 + LOSS_RTOL), tag
    if same:
        np.testing.assert_allclose(s, es, rtol=SCALE_RTOL, err_msg=tag)
    np.testing.assert_allclose(cl, ecl, rtol=LOSS_RTOL, err_msg=tag)
    assert ecl[int(round((1 - r) * 100))] <= ecl.min() * (1 + LOSS_RTOL), tag


# ------------------------------------------------------------------------------------------------ 1. spotlight cases
@pytest.mark.parametrize("route", ["array", "gram", "stats"])
@pytest.mark.parametrize("name", A.ALL_ROUTES)
def test_spotlight_cases_follow_the_oracle_on_every_route(name, route):
    """The loss lives in the named region (share >= 0.999 of ||X D||^2 for columns, exactly 1 for rows).  What the ARRAY route
    (T = 48 or 64 < 3 K: direct product X D) reaches:

    C1  K 64, N 260, uint4 g 32, columns 256..259: awq_group_diff_kernel<PIECES>, the partial second tile, its `col_ok` lanes
    C2  N 257, int8 channel symmetric, column 256: awq_diff_kernel (N % 4 == 1), scale_rows_kernel's tail, RTN at an odd width
    C3  N 258, uint4 g 8, columns 256..257: awq_diff_kernel, scale_rows_kernel's tail, groups below the fused kernel's 16 rows
    C4  K 256, N 516, int4 g 128, columns 512..515: awq_group_diff_kernel<PIECES> with 8 waves per group, the third tile
    C5  as C1, columns 0..3: the first lanes of the first tile (one row of blocks: the tile rotation (blockIdx.x + blockIdx.y) %
        gridDim.x is the identity here; C4 runs it with two rows of blocks, its region's tile taken by block 2, then block 1)
    C6  N 520, uint4 g 16, columns 256..259: the first lanes of a middle tile
    R1  K 100, N 24, int8 channel, rows 96..99: awq_diff4_kernel's K % 8 tail (clamped loads, predicated stores)
    R2  K 176, N 64, uint4 g 16, rows 160..175: awq_group_diff_kernel<no pieces> (K % 32 != 0), 11 groups at 8 per block:
        the last group next to five surplus groups that re-read group 0
    R3  K 192: the same region on the pieces route (K % 32 == 0, 12 groups)
    R4  K 64, N 64, int4 g 32 symmetric, rows 0..31: the first group, two waves per group
    R5  K 68, N 36, uint8 tensor, rows 64..67: tensor strategy (fold_to_scalar_kernel), awq_diff4_kernel's tail rows
    R6  K 256, N 64, uint4 g 128, rows 128..255: 8 waves per group, the second row of blocks

    GRAM: the same x tiled along T to T >= 3 K (loss and mean |x| unchanged): D in fp32 from the unfused kernels, <D, G D> with
    G from the Hessian kernels.  STATS: `ops.SearchStatistics` fed in two uneven batches, the statistics entry points (Gram form
    from the running Gram matrix and |x| sums).  In the row cases the channels outside the region are dead: mean |x| = 0, the
    scale clamps at 1e-4, and their rows of D carry no loss (on the fused pieces route they are written as zeros and stay out of
    the bound that sets the fp16 piece scale)."""
    ok, figures = A.meets_conditions(name)
    assert ok, figures
    c = A.spotlight(name)
    _compare(1, f"{name} {route}", _searches(route, c.x, c.w, c.qtype, c.strategy, c.g, c.sym), A.oracle(name))


@pytest.mark.parametrize("name", ["R2r", "R3r"])
def test_row_spotlights_with_the_reduced_range(name):
    """R2's and R3's shapes and regions on fresh inputs, int8 per channel with reduce_range (the grid -64 .. 64): awq_diff4_kernel
    behind the general RTN entry point, K = 176 and 192 rows, array route."""
    ok, figures = A.meets_conditions(name)
    assert ok, figures
    c = A.spotlight(name)
    assert c.reduce_range
    _compare(1, f"{name} array", _searches("array", c.x, c.w, c.qtype, c.strategy, c.g, c.sym, True), A.oracle(name))
    # the reduced range is a different search: the full range's losses are not within the bar of it
    _, full = O.awq_clip_search(c.x, c.w, c.qtype, c.strategy, c.g, c.sym, False)
    assert _deviation(full, A.oracle(name)[3]) > 10 * LOSS_RTOL


# ------------------------------------------------------------------------------------------------ the C interface
def _aligned_workspace(nbytes):
    import torch
    buf = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    off = (-buf.data_ptr()) % 256
    return buf, buf.data_ptr() + off


def _c_scale_search(xd, wd, qtype, strategy, g, sym=False, reduce_range=False, n_grid=20, workspace=None, stats=None):
    """oq_awq_scale_search_f32 (or, with `stats`, oq_awq_scale_search_stats_f32) through the loaded library: status,
    scales_out [n_grid, K], losses_out, best_out.  xd / wd may be row-strided views; `workspace` = (pointer, bytes)."""
    import torch
    from onnx_quantize_amd.hip import _lib as L
    lib = L.load()
    k, n = wd.shape
    t = stats.rows if stats is not None else xd.shape[0]
    ng = max(1, min(int(n_grid), 64))
    scales = torch.full((ng, k), -1.0, dtype=torch.float32, device="cuda")
    losses = torch.full((ng,), -1.0, dtype=torch.float32, device="cuda")
    best = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    keep = None
    if workspace is None:
        need = lib.oq_awq_stats_workspace_bytes(k, n) if stats is not None else lib.oq_awq_workspace_bytes(t, k, n)
        assert need > 0
        keep, ptr = _aligned_workspace(need)
        workspace = (ptr, need)
    tail = (L.QTYPE_CODE[qtype], L.STRATEGY_CODE[strategy], int(g), int(sym), int(reduce_range), int(n_grid), scales.data_ptr(), losses.data_ptr(),
            best.data_ptr(), C.c_void_p(workspace[0]), workspace[1], None)
    if stats is not None:
        st = lib.oq_awq_scale_search_stats_f32(stats.abs_sum.data_ptr(), stats.gram.data_ptr(), t, k, wd.data_ptr(), n, wd.stride(0), *tail)
    else:
        st = lib.oq_awq_scale_search_f32(xd.data_ptr(), t, k, xd.stride(0), wd.data_ptr(), n, wd.stride(0), *tail)
    torch.cuda.synchronize()
    del keep
    return st, scales.cpu().numpy(), losses.cpu().numpy(), int(best.item())


def _c_clip_search(xd, wd, qtype, strategy, g, sym=False, reduce_range=False, workspace=None, stats=None):
    """oq_awq_clip_search_f32 / oq_awq_clip_search_stats_f32: status, losses_out [10], best_out."""
    import torch
    from onnx_quantize_amd.hip import _lib as L
    lib = L.load()
    k, n = wd.shape
    t = stats.rows if stats is not None else xd.shape[0]
    losses = torch.full((10,), -1.0, dtype=torch.float32, device="cuda")
    best = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    keep = None
    if workspace is None:
        need = lib.oq_awq_stats_workspace_bytes(k, n) if stats is not None else lib.oq_awq_workspace_bytes(t, k, n)
        assert need > 0
        keep, ptr = _aligned_workspace(need)
        workspace = (ptr, need)
    tail = (L.QTYPE_CODE[qtype], L.STRATEGY_CODE[strategy], int(g), int(sym), int(reduce_range), losses.data_ptr(), best.data_ptr(),
            C.c_void_p(workspace[0]), workspace[1], None)
    if stats is not None:
        st = lib.oq_awq_clip_search_stats_f32(stats.gram.data_ptr(), t, k, wd.data_ptr(), n, wd.stride(0), *tail)
    else:
        st = lib.oq_awq_clip_search_f32(xd.data_ptr(), t, k, xd.stride(0), wd.data_ptr(), n, wd.stride(0), *tail)
    torch.cuda.synchronize()
    del keep
    return st, losses.cpu().numpy(), int(best.item())


# ------------------------------------------------------------------------------------------------ 2. every candidate
@pytest.mark.parametrize("n_grid", [1, 7, 20, 64])
@pytest.mark.parametrize("shape", ["C1", "K1100"])
def test_every_candidates_scale_and_the_first_minimum(shape, n_grid):
    """`scales_out` [n_grid, K], `losses_out` and `best_out` of oq_awq_scale_search_f32 and oq_awq_scale_search_stats_f32 (the `ops`
    wrappers hand out the winner's row only).  Every row is the oracle's candidate clip(act^r / ws^(1 - r), 1e-4), normalised,
    r = i / n_grid; `best_out` is NumPy's first minimum of the device's own fp32 losses; the losses meet the usual bar.
    C1's shape (uint4 g 32: fused pieces route, where the rows also feed awq_bound_kernel) and 48 x 1100 x 256, int8 per channel:
    K = 1100 is more than one lap of grid_scales_kernel's 1024 threads and of the 256-wide per-channel kernels (col_abs_partial /
    finish, weight_scale_rows), and K % 8 = 4 in awq_diff4_kernel.  (T and N of that case: tests/awq_cases.py::WIDE_SHAPE.)"""
    if shape == "C1":
        c = A.spotlight("C1")
        x, w, cfg = c.x, c.w, (c.qtype, c.strategy, c.g)
    else:
        (x, w), cfg = A.wide_channel_case(), A.WIDE_CONFIG
    xd, wd = _dev(x), _dev(w)
    want = A.candidate_scales(x, w, cfg[1], cfg[2], n_grid)
    _, el = O.awq_scale_search(x, w, *cfg, n_grid=n_grid)
    for entry, stats in (("array", None), ("stats", _statistics(xd))):
        st, scales, losses, best = _c_scale_search(xd, wd, *cfg, n_grid=n_grid, stats=stats)
        assert st == 0, (entry, st)
        print(f"AWQ-EDGE section 2 {shape} n_grid {n_grid} {entry}: loss deviation {_deviation(losses, el):.3e}, "
              f"candidate scale deviation {float(np.max(np.abs(scales / want - 1.0))):.3e}, best {best}")
        assert scales.shape == want.shape
        np.testing.assert_allclose(scales, want, rtol=SCALE_RTOL, err_msg=entry)
        assert best == int(np.argmin(losses)), (entry, best, losses)
        np.testing.assert_allclose(losses, el, rtol=LOSS_RTOL, err_msg=entry)
        assert el[best] <= el.min() * (1 + LOSS_RTOL), entry


def test_host_side_refusals_launch_nothing():
    """Each refusal returns its status and leaves the (sentinel-filled) outputs as they were."""
    import torch
    from onnx_quantize_amd.hip import _lib as L
    lib = L.load()
    c = A.spotlight("C1")
    xd, wd = _dev(c.x), _dev(c.w)
    t, k, n = 48, 64, 260
    stats = _statistics(xd)
    need, need_stats = lib.oq_awq_workspace_bytes(t, k, n), lib.oq_awq_stats_workspace_bytes(k, n)
    buf, ptr = _aligned_workspace(max(need, need_stats) + 256)

    def untouched(result):
        return all(np.all(np.asarray(v) == (-7 if np.asarray(v).dtype.kind == "i" else -1.0)) for v in result[1:])

    for stats_arg, nd in ((None, need), (stats, need_stats)):
        for n_grid in (0, 65):
            res = _c_scale_search(xd, wd, "uint4", "group", 32, n_grid=n_grid, stats=stats_arg)
            assert res[0] == L.OQ_ERR_INVALID_ARGUMENT and untouched(res), (n_grid, res[0])
        for g in (3, 48):                                  # below the smallest group; not a divisor of K = 64
            res = _c_scale_search(xd, wd, "uint4", "group", g, stats=stats_arg)
            assert res[0] == L.OQ_ERR_UNSUPPORTED and untouched(res), (g, res[0])
            res = _c_clip_search(xd, wd, "uint4", "group", g, stats=stats_arg)
            assert res[0] == L.OQ_ERR_UNSUPPORTED and untouched(res), (g, res[0])
        for workspace in ((ptr, nd - 1), (ptr + 16, nd)):   # one byte short; misaligned by 16
            res = _c_scale_search(xd, wd, "uint4", "group", 32, workspace=workspace, stats=stats_arg)
            assert res[0] == L.OQ_ERR_WORKSPACE and untouched(res), (workspace[1] - nd, res[0])
            res = _c_clip_search(xd, wd, "uint4", "group", 32, workspace=workspace, stats=stats_arg)
            assert res[0] == L.OQ_ERR_WORKSPACE and untouched(res), (workspace[1] - nd, res[0])
    x66, w66 = torch.zeros(4, 66, device="cuda"), torch.ones(66, 8, device="cuda")       # 3 divides 66: refused for its size alone
    res = _c_scale_search(x66, w66, "uint4", "group", 3)
    assert res[0] == L.OQ_ERR_UNSUPPORTED and untouched(res)
    assert lib.oq_awq_workspace_bytes(48, 65536, 64) == 0 and lib.oq_awq_stats_workspace_bytes(65536, 64) == 0
    assert lib.oq_awq_workspace_bytes(48, 65535, 64) > 0
    del buf


# ------------------------------------------------------------------------------------------------ 3. shapes and strides
@pytest.mark.parametrize("i", range(len(A.PLAIN_SHAPES)), ids=["x".join(map(str, s[:3])) for s in A.PLAIN_SHAPES])
def test_small_and_odd_shapes_follow_the_oracle(i):
    """Plain random inputs.  1 x 32 x 7 (T = 1 < kColChunks: one row chunk; uint4 g 16 at N % 4 != 0: awq_diff_kernel),
    3 x 36 x 5 (int4 g 4, the smallest group), 65 x 77 x 33 (int8 channel, all three extents odd: T one past the 64 row chunks),
    63 x 48 x 258 (uint4 g 8: scale_rows_kernel's scalar branch, awq_diff_kernel's second column block), and 191 | 192 x 64 x 12 (uint4 g 32): the two sides
    of T = 3 K -- the fused pieces route with the direct product, then the unfused group kernel with the Gram form -- on a
    12-column tile whose lanes 3..63 are `col_ok == false`."""
    t, k, n, qtype, strategy, g = A.PLAIN_SHAPES[i]
    x, w = A.plain(i)
    want = O.awq_scale_search(x, w, qtype, strategy, g) + O.awq_clip_search(x, w, qtype, strategy, g)
    _compare(3, f"{t}x{k}x{n} {qtype} {strategy} {g}", _searches("gram" if t >= 3 * k else "array", x, w, qtype, strategy, g), want)


def _strided_c1():
    """C1's operands inside wider matrices: X as xbig[:, :K] (ldx = K + 3); W as wbig[:, 4:4 + N] (ldw = N + 8, 16-byte aligned:
    the vector routes) and as wodd[:, 1:1 + N] (ldw = N + 7, misaligned: the scalar routes)."""
    import torch
    c = A.spotlight("C1")
    t, k = c.x.shape
    n = c.w.shape[1]
    xbig = torch.full((t, k + 3), 1e30, dtype=torch.float32, device="cuda")          # what lies between the rows must not be read
    wbig = torch.full((k, n + 8), 1e30, dtype=torch.float32, device="cuda")
    wodd = torch.full((k, n + 7), 1e30, dtype=torch.float32, device="cuda")
    xbig[:, :k] = _dev(c.x)
    wbig[:, 4:4 + n] = _dev(c.w)
    wodd[:, 1:1 + n] = _dev(c.w)
    xv, wv, wo = xbig[:, :k], wbig[:, 4:4 + n], wodd[:, 1:1 + n]
    assert xv.stride(0) == k + 3 and wv.stride(0) == n + 8 and wv.data_ptr() % 16 == 0 and wo.stride(0) == n + 7 and wo.data_ptr() % 16 == 4
    return c, xv, wv, wo


def test_aligned_strided_operands_give_the_bits_of_contiguous_ones():
    """ldx = K + 3, ldw = N + 8, W 16 bytes into its row: the same kernels (awq_group_diff_kernel<PIECES>, direct product) doing
    the same arithmetic in the same order as on contiguous operands -- every candidate's scale, every loss and both winners, bit
    for bit.  The same through `ops` (`_row_major` passes such views on without a copy)."""
    import torch
    from onnx_quantize_amd.hip import ops
    c, xv, wv, _ = _strided_c1()
    xd, wd = _dev(c.x), _dev(c.w)
    cfg = (c.qtype, c.strategy, c.g)
    a, b = _c_scale_search(xv, wv, *cfg), _c_scale_search(xd, wd, *cfg)
    assert a[0] == b[0] == 0 and a[3] == b[3]
    assert np.array_equal(a[1].view(np.int32), b[1].view(np.int32)) and np.array_equal(a[2].view(np.int32), b[2].view(np.int32))
    a, b = _c_clip_search(xv, wv, *cfg), _c_clip_search(xd, wd, *cfg)
    assert a[0] == b[0] == 0 and a[2] == b[2] and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    s1, l1 = ops.awq_scale_search(xv, wv, *cfg)
    s2, l2 = ops.awq_scale_search(xd, wd, *cfg)
    assert torch.equal(s1, s2) and np.array_equal(l1, l2)
    _compare(3, "C1 strided, aligned", (s1.cpu().numpy(), l1) + ops.awq_clip_search(xv, wv, *cfg), A.oracle("C1"))


def test_misaligned_strided_weights_take_the_scalar_route_and_follow_the_oracle():
    """W one element into its row with ldw = N + 7: scale_rows_kernel's scalar branch, the general RTN entry point on unaligned
    rows (the clip search quantizes W in place), awq_diff_kernel -- on C1, whose loss sits in the last four columns."""
    from onnx_quantize_amd.hip import ops
    c, xv, _, wo = _strided_c1()
    cfg = (c.qtype, c.strategy, c.g)
    s, l = ops.awq_scale_search(xv, wo, *cfg)
    _compare(3, "C1 strided, misaligned", (s.cpu().numpy(), l) + ops.awq_clip_search(xv, wo, *cfg), A.oracle("C1"))


def test_a_3d_activation_equals_its_flattened_form():
    """X as [4, T / 4, K], the way the passes hold a layer's input."""
    import torch
    from onnx_quantize_amd.hip import ops
    c = A.spotlight("C1")
    xd, wd = _dev(c.x), _dev(c.w)
    x3 = xd.reshape(4, 12, 64)
    cfg = (c.qtype, c.strategy, c.g)
    s1, l1 = ops.awq_scale_search(x3, wd, *cfg)
    s2, l2 = ops.awq_scale_search(xd, wd, *cfg)
    assert torch.equal(s1, s2) and np.array_equal(l1, l2)
    r1, c1 = ops.awq_clip_search(x3, wd, *cfg)
    r2, c2 = ops.awq_clip_search(xd, wd, *cfg)
    assert r1 == r2 and np.array_equal(c1, c2)
    _compare(3, "C1 3-D", (s1.cpu().numpy(), l1, r1, c1), A.oracle("C1"))


# ------------------------------------------------------------------------------------------------ 4. dead next to outlier
@pytest.mark.parametrize("route", ["array", "gram", "stats"])
@pytest.mark.parametrize("qtype,strategy,g", A.DEAD_OUTLIER_CONFIGS)
def test_a_dead_channel_next_to_an_outlier_channel(qtype, strategy, g, route):
    """96 x 256 x 64 with x[:, 7] = 0 and x[:, 9] *= 1000.  The dead channel's scale clamps at 1e-4 and the normalised candidate
    scales run over seven orders of magnitude (oracle: winner scales from 2e-4 to 4.5e3, losses spanning a factor of 400).  The rows
    under the outlier carry the smallest D and most of the loss.  uint4 g 32: awq_group_diff_kernel<PIECES>, whose fp16 piece scale
    comes from awq_bound_kernel's BOUND of |D| (array route), or the unfused kernel with the maximum (Gram, stats); int8 channel:
    awq_diff4_kernel, the maximum.

    As first shipped the array route of uint4 g 32 missed the bar: scale-search deviation 2.65e-3 (candidate 18; 1.9e-3 at 19).  The
    bound 2.2 max(rowmax s) / min(s) of the dead row's group took max from the outlier (s ~ 5e3) and min from the dead clamp
    (s ~ 2e-4): 5e6 against a largest |D| of 0.2, so the pieces of the outlier's rows fell into fp16's subnormals.  A CPU model of the
    pieces reproduces the figures (2.5e-3, 1.9e-3) and gives 4e-5 with dead rows left out of the bound and written as zeros, which
    is what awq_bound_kernel and awq_group_diff_kernel now do."""
    x, w = A.dead_outlier()
    want = A.dead_outlier_oracle(qtype, strategy, g)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and np.isfinite(want[3]).all()
    _compare(4, f"{qtype} {strategy} {g} {route}", _searches(route, x, w, qtype, strategy, g), want)


# ------------------------------------------------------------------------------------------------ 5. SmoothQuant
SQ_SHAPES = [(1, 32, 7), (65, 77, 5), (63, 300, 258)]


@pytest.mark.parametrize("t,k,n", SQ_SHAPES)
def test_smooth_quant_scale_shapes_alpha_zero_row_and_dead_channel(t, k, n):
    """oq_smooth_quant_scale_f32 against O.smooth_quant_scale: col_abs_partial_kernel<MAX> with T = 1 (one chunk), 65 (one row past
    64 chunks) and 63; K = 300 (a second block of the 256-wide column kernels); row_absmax_kernel at N = 5, 7 and 258 (its second
    lap).  alpha 0 (the weight term alone), 0.5, 1 (the activation term alone); one all-zero weight row (wmax + 1e-9); one dead
    activation channel (clamped to 1e-5)."""
    from onnx_quantize_amd.hip import ops
    x, w = A.inputs(500 + k, t, k, n)
    w[3, :] = 0.0
    x[:, 5] = 0.0
    xd, wd = _dev(x), _dev(w)
    for alpha in (0.0, 0.5, 1.0):
        got, want = ops.smooth_quant_scale(xd, wd, alpha).cpu().numpy(), O.smooth_quant_scale(x, w, alpha)
        assert want.dtype == np.float32 and np.isfinite(want).all()
        print(f"AWQ-EDGE section 5 {t}x{k}x{n} alpha {alpha}: deviation {float(np.max(np.abs(got / want - 1.0))):.3e}")
        np.testing.assert_allclose(got, want, rtol=SQ_RTOL, err_msg=str(alpha))
    assert want[5] == np.float32(1e-5)                                       # alpha = 1: the clamped dead channel itself


def test_smooth_quant_scale_on_strided_operands():
    """63 x 300 x 258 inside wider matrices: ldx = K + 3; W 16-byte aligned with ldw = N + 8 and misaligned with ldw = N + 7.  The
    kernels read element by element: the bits of the contiguous call, and the oracle's bar."""
    import torch
    from onnx_quantize_amd.hip import ops
    t, k, n = SQ_SHAPES[2]
    x, w = A.inputs(500 + k, t, k, n)
    xbig = torch.full((t, k + 3), 1e30, dtype=torch.float32, device="cuda")
    wbig = torch.full((k, n + 8), 1e30, dtype=torch.float32, device="cuda")
    wodd = torch.full((k, n + 7), 1e30, dtype=torch.float32, device="cuda")
    xbig[:, :k] = _dev(x)
    wbig[:, 4:4 + n] = _dev(w)
    wodd[:, 1:1 + n] = _dev(w)
    for alpha in (0.0, 0.5, 1.0):
        ref = ops.smooth_quant_scale(_dev(x), _dev(w), alpha)
        want = O.smooth_quant_scale(x, w, alpha)
        for wv in (wbig[:, 4:4 + n], wodd[:, 1:1 + n]):
            assert wv.stride(0) > n
            got = ops.smooth_quant_scale(xbig[:, :k], wv, alpha)
            assert torch.equal(got, ref), alpha
            np.testing.assert_allclose(got.cpu().numpy(), want, rtol=SQ_RTOL)


# ------------------------------------------------------------------------------------------------ 6. workspace
@pytest.mark.parametrize("name,route", [("C3", "array"), ("R1", "array"), ("C1", "gram"), ("R3", "stats")])
def test_the_searches_stay_inside_the_workspace_they_ask_for(name, route):
    """need + 2 MiB of 0xA5, the 256-byte aligned pointer 1 MiB in, `workspace_bytes` exactly oq_awq_workspace_bytes (or
    oq_awq_stats_workspace_bytes): after both searches and a synchronise the two 1 MiB guard bands are untouched, and the results
    are the bits of the `ops` call (whose workspace holds other bytes: nothing reads what it did not write).  C3: general route,
    scalar kernels; R1: awq_diff4_kernel; C1 tiled: Gram route (G, its pieces, the Hessian workspace); R3: statistics entry."""
    import torch
    from onnx_quantize_amd.hip import _lib as L
    from onnx_quantize_amd.hip import ops
    lib = L.load()
    c = A.spotlight(name)
    cfg = (c.qtype, c.strategy, c.g, c.sym)
    wd = _dev(c.w)
    xd = _dev(A.tiled_for_gram(c.x, c.x.shape[1]) if route == "gram" else c.x)
    t, k = xd.shape
    n = wd.shape[1]
    stats = _statistics(xd) if route == "stats" else None
    need = lib.oq_awq_stats_workspace_bytes(k, n) if stats is not None else lib.oq_awq_workspace_bytes(t, k, n)
    assert need > 0
    buf = torch.full((need + 2 * MIB,), 0xA5, dtype=torch.uint8, device="cuda")
    ptr = buf.data_ptr() + MIB
    assert ptr % 256 == 0
    st, scales, losses, best = _c_scale_search(xd, wd, *cfg, workspace=(ptr, need), stats=stats)
    st2, closses, cbest = _c_clip_search(xd, wd, *cfg, workspace=(ptr, need), stats=stats)
    torch.cuda.synchronize()
    assert st == 0 and st2 == 0
    assert bool((buf[:MIB] == 0xA5).all()) and bool((buf[MIB + need:] == 0xA5).all()), "a search wrote outside its workspace"
    assert buf[MIB + need:].numel() == MIB
    if stats is not None:
        s, l = ops.awq_scale_search_stats(stats, wd, *cfg)
        r, cl = ops.awq_clip_search_stats(stats, wd, *cfg)
    else:
        s, l = ops.awq_scale_search(xd, wd, *cfg)
        r, cl = ops.awq_clip_search(xd, wd, *cfg)
    assert np.array_equal(losses.astype(np.float64), l) and np.array_equal(scales[best], s.cpu().numpy())
    assert np.array_equal(closses.astype(np.float64), cl) and r == 1 - cbest / 100
