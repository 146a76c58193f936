"""`oq_gptq_loop_f32` in corrected mode against a plain float64 loop, byte for byte (tests/gptq_loop_cases.py has the argument and the
recipes, tests/test_gptq_loop_cases.py checks them on the host).

On the exact cases every operation of the loop is exact in fp32, so the integers, the dequantized values, the parameters in force
and the final working matrix do not depend on the summation order, the blocking, the kernel (rows over lanes or one column per
lane) or the route of an update product (in-launch registers, panel update or its fp32 fallback, deferred fp32 GEMM or fp16 pieces):
the kernels owe `restate`'s bytes.  The fp32 family (random floats, U confined to each launch's own diagonal block) holds the same
five outputs to an fp32 numpy loop with the kernels' roundings.  A failure names the launch, slab, lane and column (`describe`)."""
import ctypes as C

import numpy as np
import pytest
import torch

import oq_oracle as O
import gptq_loop_cases as G

pytestmark = pytest.mark.gpu

MODES = ("corrected", "corrected_columns")
SENTINEL, GUARD = 0x5C, 256


@pytest.fixture(scope="module")
def ops():
    from onnx_quantize_amd.hip import ops
    return ops


def run(ops, c, mode, layout="kn", method=None, w=None):
    """-> dict of host arrays: q (bytes), q_deq, used_scale, used_zp, w (the working matrix after the call)"""
    W = torch.from_numpy(np.array(c.w if w is None else w)).cuda()
    U = torch.from_numpy(c.u).cuda()
    q, qd, us, uz = ops.gptq_loop(W, U, c.qtype, c.g, c.symmetric, c.reduce_range, 1.0, False, c.block_size, mode,
                                  torch.from_numpy(c.init_scale).cuda(), torch.from_numpy(c.init_zp).cuda(), want_used=True, layout=layout,
                                  method=method)
    torch.cuda.synchronize()
    return dict(q=q.cpu().numpy().view(np.uint8), q_deq=qd.cpu().numpy(), used_scale=None if us is None else us.cpu().numpy(),
                used_zp=None if uz is None else uz.cpu().numpy(), w=W.cpu().numpy())


def want_of(c, res, layout="kn"):
    K, N = c.w.shape
    q = res.q.astype(O.container_dtype(c.qtype)).view(np.uint8)
    if layout == "kn_packed4":
        q = O.pack_nibbles(res.q).reshape(K, N // 2)
    return dict(q=q, q_deq=res.q_deq.astype(np.float32), used_scale=None if res.used_scale is None else res.used_scale.astype(np.float32),
                used_zp=None if res.used_zp is None else res.used_zp.astype(np.int32), w=res.w.astype(np.float32))


def assert_bytes(got, want, c, mode, layout="kn", skip_columns=()):
    K, N = c.w.shape
    keep = np.ones(N, dtype=bool)
    keep[list(skip_columns)] = False
    for name in ("q", "q_deq", "used_scale", "used_zp", "w"):
        g, w = got[name], want[name]
        assert (g is None) == (w is None), name
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape, g.dtype, w.dtype)
        if name == "q" and layout == "kn_packed4":
            wrong = np.repeat(g != w, 2, axis=1)
        else:
            wrong = g.view(np.uint8).reshape(g.shape[0], N, -1) != w.view(np.uint8).reshape(w.shape[0], N, -1)
            wrong = wrong.any(axis=2)
        wrong = wrong & keep[None, :]
        if wrong.any():
            if name in ("used_scale", "used_zp"):               # a row per group: name the group's first row
                rows = np.zeros((K, N), dtype=bool)
                rows[np.arange(wrong.shape[0]) * c.g] = wrong
                wrong = rows
            r, cc = np.argwhere(wrong)[0]
            pytest.fail(f"{c.name} [{mode}] {name}: " + G.describe(wrong, K, N, c.g, c.block_size, mode) +
                        f"; first at ({r}, {cc})")


def check(ops, name, mode, layout="kn", method=None):
    c, res = G.restated(name)
    assert_bytes(run(ops, c, mode, layout, method), want_of(c, res, layout), c, mode, layout)


# ------------------------------------------------------------------------------------ one launch
ONE = [n for n in G.CASES if n.startswith(("one-", "wide-"))]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ONE)
def test_one_launch(ops, name, mode):
    """K in {1, 15, 16, 17, 100, 127, 128} x N in {1, 3, 4, 5, 16, 17, 63, 64, 65, 130}: a dense 8-bit U, the initial parameters per
    column or one for all; N = 4100 and 12292 at K = 32, where a rows-over-lanes workgroup takes 8 and 16 waves."""
    check(ops, name, mode)


# ------------------------------------------------------------------------------------ several launches, every update leg
MULTI = [n for n in G.CASES if n.startswith("multi-")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", MULTI)
def test_multi_launch(ops, name, mode):
    check(ops, name, mode)


@pytest.mark.parametrize("mode,method", [("corrected", None), ("corrected", "f32"), ("corrected_columns", None)])
def test_deferred_legs(ops, mode, method):
    """(K, N) = (1536, 1024): the product behind the first super-block has M N = 2^20 and runs on the fp16 pieces, the one behind
    the second on the fp32 GEMM; method = f32 keeps both there.  The same bytes."""
    check(ops, "deferred-1536x1024", mode, method=method)


# ------------------------------------------------------------------------------------ types, grids, the packed layout
TYPED = [n for n in G.CASES if n.startswith("type-")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", TYPED)
def test_types_and_grids(ops, name, mode):
    check(ops, name, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", G.PACKED_CASES)
def test_packed_nibbles(ops, name, mode):
    assert G.SHAPES[name][1] % 2 == 0
    check(ops, name, mode, layout="kn_packed4")


# ------------------------------------------------------------------------------------ which version of W a group's parameters see
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", G.VERSION_CASES)
def test_parameter_versions(ops, name, mode):
    """A group's scale is s where the reference reads its rows before a probe's error has reached W and 2 s after
    (tests/gptq_loop_cases.py: `exact_case(versions=...)`)."""
    c, res = G.restated(name)
    got = run(ops, c, mode)
    for tgt, f in G.expected_versions(c).items():
        assert np.array_equal(got["used_scale"][tgt], (f * c.scale).astype(np.float32)), \
            f"{name} [{mode}]: group {tgt} must see the scale x {f}, got x {np.unique(got['used_scale'][tgt] / c.scale)}"
    assert_bytes(got, want_of(c, res), c, mode)


# ------------------------------------------------------------------------------------ fp32 roundings
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", G.FP32_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_family(ops, shape, mode):
    """Random floats; every update product adds exact zeros, so the kernels owe an fp32 numpy loop bit for bit: IEEE divide, rint,
    one rounding for the product and one for the subtraction.  used_scale / used_zp are `O.qparams` on the rows the reference reads."""
    K, N, g, bs = shape
    w, u, s, z = G.fp32_case(K, N, g, bs)
    res = G.restate(w, u, "uint8", g, bs, False, False, s, z, dtype=np.float32)
    c = G.Case(f"fp32-{K}x{N}", w, u, "uint8", g, bs, False, False, s, z, None, None, None, None, None, None, ())
    assert_bytes(run(ops, c, mode), want_of(c, res), c, mode)


@pytest.mark.parametrize("mode", MODES)
def test_products_are_rounded_before_the_subtraction(ops, mode):
    """gptq.py:198-200 is a matmul and a subtraction: two roundings.  On `contraction_case` a fused multiply-add in the row update
    moves every target row up by one level."""
    w, u, s, z, targets = G.contraction_case()
    K, N = w.shape
    res = G.restate(w, u, "uint8", 0, 128, False, False, s, z, dtype=np.float32)
    c = G.Case("contraction", w, u, "uint8", 0, 128, False, False, s, z, None, None, None, None, None, None, ())
    assert_bytes(run(ops, c, mode), want_of(c, res), c, mode)


# ------------------------------------------------------------------------------------ containment
@pytest.mark.parametrize("mode", MODES)
def test_a_nan_stays_in_its_column(ops, mode):
    name, col = "multi-384-128-64-52", 7
    c, res = G.restated(name)
    w = c.w.copy()
    w[5, col] = np.nan
    got = run(ops, c, mode, w=w)
    assert np.isnan(got["w"][:, col]).any()
    assert_bytes(got, want_of(c, res), c, mode, skip_columns=(col,))


@pytest.mark.parametrize("mode", MODES)
def test_sentinels_around_every_output_survive(ops, mode):
    """256 sentinel bytes either side of q_int, q_deq, used_scale, used_zp and W at ragged K and N; the outputs between them are
    `restate`'s."""
    from onnx_quantize_amd.hip import _lib as L
    lib = L.load()
    name = "multi-200-64-16-130"
    c, res = G.restated(name)
    K, N = c.w.shape
    ng = G.ceil_div(K, c.g)
    sizes = dict(q=K * N, q_deq=K * N * 4, used_scale=ng * N * 4, used_zp=ng * N * 4, w=K * N * 4)
    bufs, ptrs = {}, {}
    for k, n in sizes.items():
        b = torch.full((n + 2 * GUARD + 256,), SENTINEL, dtype=torch.uint8, device="cuda")
        start = (-b.data_ptr()) % 256 + GUARD
        bufs[k], ptrs[k] = (b, start), b.data_ptr() + start
    bufs["w"][0][bufs["w"][1]:bufs["w"][1] + sizes["w"]] = torch.from_numpy(c.w.view(np.uint8).reshape(-1)).cuda()
    U = torch.from_numpy(c.u).cuda()
    s0, z0 = torch.from_numpy(c.init_scale).cuda(), torch.from_numpy(c.init_zp).cuda()
    need = lib.oq_gptq_loop_workspace_bytes(K, N, c.block_size)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    st = lib.oq_gptq_loop_f32(C.c_void_p(ptrs["w"]), K, N, C.c_void_p(U.data_ptr()), L.QTYPE_CODE[c.qtype], c.g, 0, 0, 1.0, 0, c.block_size,
                              ops._LOOP_MODES[mode], 0, C.c_void_p(s0.data_ptr()), C.c_void_p(z0.data_ptr()), N, C.c_void_p(ptrs["q"]),
                              L.OQ_LAYOUT_KN, C.c_void_p(ptrs["q_deq"]), C.c_void_p(ptrs["used_scale"]), C.c_void_p(ptrs["used_zp"]),
                              C.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256), need, None)
    torch.cuda.synchronize()
    assert st == 0, lib.oq_last_error().decode()
    want = want_of(c, res)
    got = {}
    for k, (b, start) in bufs.items():
        host = b.cpu().numpy()
        assert (host[:start] == SENTINEL).all() and (host[start + sizes[k]:] == SENTINEL).all(), f"{k}: a sentinel byte was written"
        got[k] = host[start:start + sizes[k]].copy().view(want[k].dtype).reshape(want[k].shape)
    assert_bytes(got, want, c, mode)
