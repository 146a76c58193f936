"""The AWQ / SmoothQuant searches straight from fp16 / bf16 weights (the `_h16` entry points of include/oq_hip_half.h, csrc/awq.hip
as templates on the element type).

DEFINITION: the result is that of the `_f32` entry point on the upcast matrix -- every candidate scale (`scales_out` as a whole),
every loss, the winner, the clip ratio and the SmoothQuant scale, byte for byte, NaN patterns included.  The comparisons below
call the C entry points themselves (ctypes), because `ops` hands out the winning row only; the fp32 twin gets the upcast matrix
in the SAME layout (leading dimension, element offset), so both sides take the same route through the kernels.

Shapes are the smallest that reach an edge of a route (tests/awq_cases.py, tests/test_awq_edges_gpu.py name them):
  fused pieces route   array x, T < 3 K, group 16 / 32 / 128: 96 x 256 x 64; K = 160 (five groups: a surplus group in the last
                       block); N = 260 (a partial last column tile); the dead channel next to an outlier channel
  fused without pieces the same shapes from running statistics (the Gram route)
  awq_diff4_kernel     int8 per channel and per tensor at 48 x 1100 x 256 (a partial last block of 8 rows)
  scalar kernels       N = 7; a view with an odd leading dimension; a base that is only 2-byte aligned"""
import ctypes as C

import numpy as np
import pytest

from awq_cases import dead_outlier, inputs, wide_channel_case

pytestmark = pytest.mark.gpu

DTYPES = ["float16", "bfloat16"]
SENTINEL = -12345.0


def _dt(name):
    import torch
    return getattr(torch, name)


def _lib():
    from onnx_quantize_amd.hip import _lib as L
    return L, L.load()


def _aligned(nbytes):
    import torch
    t = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device="cuda")
    return t, t.data_ptr() + (-t.data_ptr()) % 256


def _w_args(w):
    """(pointer[, wtype]), suffix, leading dimension of a 2-D tensor whose rows are contiguous."""
    import torch
    assert w.dim() == 2 and w.stride(1) == 1
    ldw = w.stride(0) if w.shape[0] > 1 else w.shape[1]
    if w.dtype == torch.float32:
        return (C.c_void_p(w.data_ptr()),), "f32", ldw
    return (C.c_void_p(w.data_ptr()), 0 if w.dtype == torch.float16 else 1), "h16", ldw


def _stats(x):
    from onnx_quantize_amd.hip import ops
    st = ops.SearchStatistics(x.shape[1], "cuda")
    st.add(x)
    return st


def _search(which, x, w, cfg, n_grid=20):
    """One C call: `which` in scale / clip / scale_stats / clip_stats; `x` an fp32 [T, K] tensor or SearchStatistics.
    Returns the outputs as int32 views (bytes): (scales or None, losses, best)."""
    import torch
    L, lib = _lib()
    qtype, strategy, g, sym, rr = cfg
    k, n = w.shape
    wargs, kind, ldw = _w_args(w)
    stats = which.endswith("_stats")
    if stats:
        query = lib.oq_awq_stats_half_workspace_bytes if kind == "h16" else lib.oq_awq_stats_workspace_bytes
        need = query(k, n)
    else:
        query = lib.oq_awq_half_workspace_bytes if kind == "h16" else lib.oq_awq_workspace_bytes
        need = query(x.shape[0], k, n)
    assert need > 0
    keep, ws = _aligned(need)
    count = n_grid if which.startswith("scale") else 10
    scales = torch.full((n_grid, k), SENTINEL, dtype=torch.float32, device="cuda")
    losses = torch.full((count,), SENTINEL, dtype=torch.float32, device="cuda")
    best = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    tail = [L.QTYPE_CODE[qtype], L.STRATEGY_CODE[strategy], -1 if g is None else g, int(sym), int(rr)]
    out = [C.c_void_p(losses.data_ptr()), C.c_void_p(best.data_ptr()), C.c_void_p(ws), need, None]
    if which.startswith("scale"):
        out = [n_grid, C.c_void_p(scales.data_ptr())] + out
    if which == "scale_stats":
        head = [C.c_void_p(x.abs_sum.data_ptr()), C.c_void_p(x.gram.data_ptr()), x.rows, k]
    elif which == "clip_stats":
        head = [C.c_void_p(x.gram.data_ptr()), x.rows, k]
    else:
        assert x.dtype == torch.float32 and x.is_contiguous()
        head = [C.c_void_p(x.data_ptr()), x.shape[0], k, k]
    fn = getattr(lib, f"oq_awq_{which.replace('_stats', '')}_search{'_stats' if stats else ''}_{kind}")
    L.check(fn(*head, *wargs, n, ldw, *tail, *out))
    torch.cuda.synchronize()
    del keep
    return (scales.view(torch.int32) if which.startswith("scale") else None), losses.view(torch.int32), int(best.item())


def _same(a, b, what):
    import torch
    if a is None:
        assert b is None
        return
    assert torch.equal(a, b), (what, int((a != b).sum()))


def _compare(x, wh, w32, cfg, routes=("array", "stats"), n_grid=20):
    """Both searches on the given routes: the half entry against the fp32 entry on the upcast matrix, as bytes."""
    import torch
    assert w32.dtype == torch.float32 and torch.equal(w32, wh.float()) or bool(torch.isnan(w32).any())
    for route in routes:
        src = x if route == "array" else _stats(x)
        for which in ("scale", "clip"):
            name = which + ("_stats" if route == "stats" else "")
            got, ref = _search(name, src, wh, cfg, n_grid), _search(name, src, w32, cfg, n_grid)
            _same(got[0], ref[0], (name, "scales"))
            _same(got[1], ref[1], (name, "losses"))
            assert got[2] == ref[2], (name, "best", got[2], ref[2])
            assert not (got[1] == torch.tensor(SENTINEL).view(torch.int32).item()).any()


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a)).cuda()                  # a copy: the shared cases are read-only
    return t if dtype is None else t.to(_dt(dtype))


# ------------------------------------------------------------------------------------ the fused group route, with and without pieces
U4 = lambda g: ("uint4", "group", g, False, False)      # noqa: E731
FUSED = {
    "96x256x64 g32": (96, 256, 64, 32), "K=160: a surplus group": (96, 160, 64, 32), "N=260: a partial column tile": (96, 256, 260, 32),
    "g16": (96, 256, 64, 16), "g128": (96, 256, 64, 128),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(FUSED), ids=list(FUSED))
def test_fused_group_route_gives_the_bytes_of_the_upcast(case, dtype):
    t, k, n, g = FUSED[case]
    x, w = inputs(20, t, k, n)
    wh = _dev(w, dtype)
    _compare(_dev(x), wh, wh.float(), U4(g))


@pytest.mark.parametrize("dtype", DTYPES)
def test_dead_channel_next_to_an_outlier_gives_the_bytes_of_the_upcast(dtype):
    x, w = dead_outlier()                                       # x[:, 7] = 0, x[:, 9] *= 1000 at 96 x 256 x 64
    wh = _dev(w, dtype)
    _compare(_dev(x), wh, wh.float(), U4(32))


# ------------------------------------------------------------------------------------ the four-column difference kernel
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("strategy", ["channel", "tensor"])
def test_diff4_kernel_gives_the_bytes_of_the_upcast(strategy, dtype):
    x, w = wide_channel_case()                                  # 48 x 1100 x 256: 1100 = 137 * 8 + 4
    wh = _dev(w, dtype)
    _compare(_dev(x), wh, wh.float(), ("int8", strategy, None, False, False))


# ------------------------------------------------------------------------------------ the one-column kernels
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", [U4(16), ("int8", "channel", None, False, False)], ids=["group16", "channel"])
def test_seven_columns_take_the_scalar_kernels(cfg, dtype):
    x, w = inputs(21, 48, 64, 7)
    wh = _dev(w, dtype)
    _compare(_dev(x), wh, wh.float(), cfg)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", [U4(32), ("int8", "channel", None, False, False)], ids=["group32", "channel"])
def test_a_view_with_an_odd_leading_dimension(cfg, dtype):
    """64 of 67 columns: N % 4 == 0 but rows that are only 2-byte aligned.  The fp32 twin reads the same view of the upcast."""
    x, w = inputs(22, 48, 64, 67)
    big = _dev(w, dtype)
    big32 = big.float()
    wh, w32 = big[:, :64], big32[:, :64]
    assert wh.stride(0) == 67 and w32.stride(0) == 67
    _compare(_dev(x), wh, w32, cfg)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", [U4(32), ("int8", "channel", None, False, False)], ids=["group32", "channel"])
def test_a_base_that_is_only_two_byte_aligned(cfg, dtype):
    """Contiguous [64, 64] one element into a buffer: N and ldw are multiples of four, the base is not 8-byte aligned."""
    import torch
    x, w = inputs(23, 48, 64, 64)
    flat = torch.zeros(64 * 64 + 8, dtype=_dt(dtype), device="cuda")
    flat32 = torch.zeros(64 * 64 + 8, dtype=torch.float32, device="cuda")
    wh = flat[1:1 + 64 * 64].view(64, 64)
    wh.copy_(_dev(w, dtype))
    w32 = flat32[1:1 + 64 * 64].view(64, 64)
    w32.copy_(wh.float())
    assert wh.data_ptr() % 8 == 2 and w32.data_ptr() % 16 == 4
    _compare(_dev(x), wh, w32, cfg)
    # the same matrix at an aligned base takes the vector kernels: the same bytes again
    wa = wh.clone()
    assert wa.data_ptr() % 16 == 0
    for which in ("scale", "clip"):
        a, b = _search(which, _dev(x), wh, cfg), _search(which, _dev(x), wa, cfg)
        _same(a[0], b[0], which)
        _same(a[1], b[1], which)
        assert a[2] == b[2]


# ------------------------------------------------------------------------------------ n_grid
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_grid", [1, 7, 64])
def test_grid_sizes(n_grid, dtype):
    x, w = inputs(20, 96, 256, 64)
    wh = _dev(w, dtype)
    xd = _dev(x)
    for name, src in (("scale", xd), ("scale_stats", _stats(xd))):
        got, ref = _search(name, src, wh, U4(32), n_grid), _search(name, src, wh.float(), U4(32), n_grid)
        _same(got[0], ref[0], name)
        _same(got[1], ref[1], name)
        assert got[2] == ref[2] and 0 <= got[2] < n_grid


# ------------------------------------------------------------------------------------ special values
def _specials(dtype, with_nan):
    """96 x 256 x 64 with the extremes of the element type in the first, a middle and the last row of a group of 32."""
    import torch
    x, w = inputs(24, 96, 256, 64)
    wh = _dev(w, dtype)
    big = 65504.0 if dtype == "float16" else 3.39e38
    tiny = 2.0 ** -24 if dtype == "float16" else 2.0 ** -133          # a subnormal of the type
    for row, col in ((32, 0), (45, 1), (63, 2)):                      # group 1 of 32 rows: first, middle, last
        wh[row, col] = big
        wh[row, col + 4] = -big
        wh[row, col + 8] = tiny
        wh[row, col + 12] = -tiny
        wh[row, col + 16] = 0.0
        wh[row, col + 20] = -0.0
    assert float(wh[32, 8]) == tiny and float(wh[32, 0]) == pytest.approx(big, rel=1e-2)
    assert bool(torch.signbit(wh[32, 20]))
    if with_nan:
        for row, col in ((64, 30), (77, 31), (95, 32)):               # group 2
            wh[row, col] = float("nan")
    return _dev(x), wh


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_nan", [False, True], ids=["finite", "nan"])
@pytest.mark.parametrize("cfg", [U4(32), ("int8", "channel", None, False, False)], ids=["group32", "channel"])
def test_special_values_give_the_bytes_and_the_nan_pattern_of_the_upcast(cfg, with_nan, dtype):
    import torch
    x, wh = _specials(dtype, with_nan)
    w32 = wh.float()
    assert bool(torch.isnan(w32).any()) == with_nan
    _compare(x, wh, w32, cfg)
    from onnx_quantize_amd.hip import ops
    a, b = ops.smooth_quant_scale(x, wh, 0.5), ops.smooth_quant_scale(x, w32, 0.5)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert bool(torch.isnan(a).any()) == with_nan


# ------------------------------------------------------------------------------------ SmoothQuant, and the public functions
@pytest.mark.parametrize("dtype", DTYPES)
def test_ops_dispatch_half_weights_and_views(dtype):
    """The six public functions take the half weight as it is -- contiguous, and a view with a leading dimension."""
    import torch
    from onnx_quantize_amd.hip import ops
    x, w = inputs(25, 96, 256, 68)
    xd, big = _dev(x), _dev(w, dtype)
    st = _stats(xd)
    for wh in (big[:, :64].contiguous(), big[:, :64], big[:, 1:65]):
        w32 = wh.float()
        s, l = ops.awq_scale_search(xd, wh, "uint4", "group", 32)
        s2, l2 = ops.awq_scale_search(xd, w32, "uint4", "group", 32)
        assert torch.equal(s, s2) and np.array_equal(l, l2)
        r, cl = ops.awq_clip_search(xd, wh, "uint4", "group", 32)
        r2, cl2 = ops.awq_clip_search(xd, w32, "uint4", "group", 32)
        assert r == r2 and np.array_equal(cl, cl2)
        s, l = ops.awq_scale_search_stats(st, wh, "int8", "channel", None)
        s2, l2 = ops.awq_scale_search_stats(st, w32, "int8", "channel", None)
        assert torch.equal(s, s2) and np.array_equal(l, l2)
        r, cl = ops.awq_clip_search_stats(st, wh, "int8", "channel", None)
        r2, cl2 = ops.awq_clip_search_stats(st, w32, "int8", "channel", None)
        assert r == r2 and np.array_equal(cl, cl2)
        assert torch.equal(ops.smooth_quant_scale(xd, wh, 0.5), ops.smooth_quant_scale(xd, w32, 0.5))
        assert torch.equal(ops.smooth_quant_scale_stats(st, wh, 0.3), ops.smooth_quant_scale_stats(st, w32, 0.3))
    with pytest.raises(TypeError):
        ops.awq_scale_search(xd, big.double(), "uint4", "group", 32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_general_clip_route_on_tall_groups_uses_the_half_rtn(dtype):
    """group 512 of K = 1024 (taller than the fused kernel's 128 and than the half RTN's one-launch 256) and group 8: the clip search
    quantizes the 2-byte W itself through oq_rtn_quantize_h16 and its workspace."""
    x, w = inputs(26, 48, 1024, 64)
    wh = _dev(w, dtype)
    for g in (512, 8):
        _compare(_dev(x), wh, wh.float(), U4(g), routes=("array",))


# ------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("dtype", DTYPES)
def test_half_weight_searches_follow_the_oracle(dtype):
    """The bars of tests/test_preprocessing.py (losses 2e-3, the chosen grid point optimal within that), the oracle on the upcast
    inputs of test_search_stats_half_gpu._search_inputs: _inputs(5, 768, 256, 192), activations and weight rounded to the type."""
    import oq_oracle as O
    import torch
    from onnx_quantize_amd.hip import ops
    r = np.random.default_rng(5)
    x = r.standard_normal((4, 192, 256)).astype(np.float32) * r.uniform(0.1, 4, 256).astype(np.float32)
    w = (r.standard_normal((256, 192)) * 0.05).astype(np.float32)
    xh = torch.from_numpy(x).cuda().to(_dt(dtype)).reshape(768, 256)
    wh = torch.from_numpy(w).cuda().to(_dt(dtype))
    x_up, w_up = xh.float().cpu().numpy(), wh.float().cpu().numpy()
    stats = ops.SearchStatistics(256, "cuda")
    stats.add(xh)
    es, el = O.awq_scale_search(x_up, w_up, "uint4", "group", 32)
    er, ecl = O.awq_clip_search(x_up, w_up, "uint4", "group", 32)
    for s, l in (ops.awq_scale_search_stats(stats, wh, "uint4", "group", 32), ops.awq_scale_search(xh.float(), wh, "uint4", "group", 32)):
        np.testing.assert_allclose(l, el, rtol=2e-3)
        assert el[int(np.argmin(l))] <= el.min() * (1 + 2e-3)
        if int(np.argmin(l)) == int(np.argmin(el)):
            np.testing.assert_allclose(s.cpu().numpy(), es, rtol=2e-5)
    for rr, cl in (ops.awq_clip_search_stats(stats, wh, "uint4", "group", 32), ops.awq_clip_search(xh.float(), wh, "uint4", "group", 32)):
        np.testing.assert_allclose(cl, ecl, rtol=2e-3)
        assert ecl[int(round((1 - rr) * 100))] <= ecl.min() * (1 + 2e-3)
    np.testing.assert_allclose(ops.smooth_quant_scale(xh.float(), wh, 0.5).cpu().numpy(), O.smooth_quant_scale(x_up, w_up, 0.5), rtol=2e-5)


# ------------------------------------------------------------------------------------ no fp32 copy
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_fp32_copy_of_the_weight_is_made(dtype):
    """2048 x 2048: the half weight is 8 MB, its fp32 copy would be 16 MB.  After a warm call of each (the scratch arena exists from
    then on), the statistics search on the half weight may allocate what the same search on an fp32 weight allocates plus less than
    4 bytes per element of W -- it allocates the 1.3 MB of partial ranges the general clip route would use."""
    import torch
    from onnx_quantize_amd.hip import ops
    k = n = 2048
    r = np.random.default_rng(7)
    w32 = _dev((r.standard_normal((k, n)) * 0.05).astype(np.float32))
    wh = w32.to(_dt(dtype))
    stats = _stats(_dev(r.standard_normal((64, k)).astype(np.float32)))

    def rise(w):
        ops.awq_scale_search_stats(stats, w, "uint4", "group", 128)           # warm
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        ops.awq_scale_search_stats(stats, w, "uint4", "group", 128)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    ops.awq_scale_search_stats(stats, wh, "uint4", "group", 128)              # the arena grows to the larger (half) request first
    full = rise(w32)
    half = rise(wh)
    print(f"rise of max_memory_allocated: fp32 weight {full}, {dtype} weight {half}, 4 bytes per element {4 * k * n}")
    assert half - full < 4 * k * n, (half, full)


# ------------------------------------------------------------------------------------ refusals
def _refusal_calls():
    """name -> (entry point, argument list builder(overrides), outputs).  Every pointer is real device memory of the right size for
    the base case 16 x 64 x 8, group 16."""
    import torch
    L, lib = _lib()
    t, k, n = 16, 64, 8
    x = torch.randn(t, k, device="cuda")
    w = torch.randn(k, n, device="cuda").half()
    gram = torch.eye(k, device="cuda")
    act = torch.ones(k, device="cuda")
    need = max(lib.oq_awq_half_workspace_bytes(t, k, n), lib.oq_awq_stats_half_workspace_bytes(k, n), lib.oq_smooth_quant_workspace_bytes(k))
    keep, ws = _aligned(need)
    outs = dict(scales=torch.full((64, k), SENTINEL, device="cuda"), losses=torch.full((64,), SENTINEL, device="cuda"),
                best=torch.full((1,), -7, dtype=torch.int32, device="cuda"), scale=torch.full((k,), SENTINEL, device="cuda"))
    p = lambda v: C.c_void_p(v.data_ptr())      # noqa: E731
    base = dict(X=p(x), T=t, K=k, ldx=k, act=p(act), G=p(gram), W=w.data_ptr(), wtype=0, N=n, ldw=n, qtype=1, strategy=2, g=16, sym=0, rr=0,
                n_grid=20, scales=p(outs["scales"]), losses=p(outs["losses"]), best=p(outs["best"]), scale=p(outs["scale"]), ws=ws,
                ws_bytes=need, alpha=0.5)
    order = {
        "oq_awq_scale_search_h16": "X T K ldx W wtype N ldw qtype strategy g sym rr n_grid scales losses best ws ws_bytes",
        "oq_awq_clip_search_h16": "X T K ldx W wtype N ldw qtype strategy g sym rr losses best ws ws_bytes",
        "oq_awq_scale_search_stats_h16": "act G T K W wtype N ldw qtype strategy g sym rr n_grid scales losses best ws ws_bytes",
        "oq_awq_clip_search_stats_h16": "G T K W wtype N ldw qtype strategy g sym rr losses best ws ws_bytes",
        "oq_smooth_quant_scale_h16": "X T K ldx W wtype N ldw alpha scale ws ws_bytes",
    }

    def call(name, **over):
        a = dict(base)
        a.update(over)
        args = [C.c_void_p(a[f]) if f in ("W", "ws") else a[f] for f in order[name].split()]
        return getattr(lib, name)(*args, None)

    return call, outs, order, base, (keep, x, w, gram, act)


AWQ_ENTRIES = ["oq_awq_scale_search_h16", "oq_awq_clip_search_h16", "oq_awq_scale_search_stats_h16", "oq_awq_clip_search_stats_h16"]
REFUSALS = [
    ("unknown wtype", dict(wtype=2), -1, None), ("negative wtype", dict(wtype=-1), -1, None), ("odd W pointer", "odd", -1, None),
    ("n_grid 0", dict(n_grid=0), -1, "scale"), ("n_grid 65", dict(n_grid=65), -1, "scale"),
    ("group 3", dict(g=3), -2, "awq"), ("group 24 does not divide 64", dict(g=24), -2, "awq"),
    ("short workspace", "short", -3, None), ("misaligned workspace", "misaligned", -3, "awq"), ("no workspace", dict(ws=0), -3, None),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_leave_every_output_untouched(case):
    import torch
    _, over, status, only = case
    call, outs, order, base, keep = _refusal_calls()
    before = {k: v.clone() for k, v in outs.items()}
    for name in order:
        if only == "awq" and name not in AWQ_ENTRIES or only == "scale" and "scale_search" not in name:
            continue
        if over == "odd":
            o = dict(W=base["W"] + 1)
        elif over == "short":
            o = dict(ws_bytes=1024)
        elif over == "misaligned":
            o = dict(ws=base["ws"] + 64)
        else:
            o = over
        got = call(name, **o)
        assert got == status, (name, got)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert torch.equal(v, before[k]), k


def test_k_65536_is_refused_before_any_launch():
    import torch
    L, lib = _lib()
    k, n = 65536, 4
    x = torch.zeros(1, k, device="cuda")
    w = torch.zeros(k, n, dtype=torch.float16, device="cuda")
    losses = torch.full((64,), SENTINEL, device="cuda")
    scales = torch.full((1, k), SENTINEL, device="cuda")
    best = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    keep, ws = _aligned(1 << 20)
    p = lambda v: C.c_void_p(v.data_ptr())      # noqa: E731
    assert lib.oq_awq_half_workspace_bytes(1, k, n) == 0 and lib.oq_awq_stats_half_workspace_bytes(k, n) == 0
    st = lib.oq_awq_scale_search_h16(p(x), 1, k, k, p(w), 0, n, n, 1, 2, 128, 0, 0, 1, p(scales), p(losses), p(best), C.c_void_p(ws), 1 << 20, None)
    assert st == -2, st
    st = lib.oq_awq_clip_search_h16(p(x), 1, k, k, p(w), 0, n, n, 1, 2, 128, 0, 0, p(losses), p(best), C.c_void_p(ws), 1 << 20, None)
    assert st == -2, st
    torch.cuda.synchronize()
    assert bool((losses == SENTINEL).all()) and bool((scales == SENTINEL).all()) and int(best.item()) == -7
