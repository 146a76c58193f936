"""Workspaces of exactly the advertised size.  For seven entry points, one raw call each through `_lib` with

  * a workspace that is a slice of exactly `need` bytes (the entry point's own query) of a larger device buffer,
  * starting at the least alignment the entry point accepts -- 8 bytes behind a 256-byte boundary for those that take any base,
    on the boundary for `oq_matmul_nbits` and `oq_qlinear_matmul`, which demand it --,
  * with 256 guard bytes of a fixed pattern on either side.

Afterwards the guards are intact, the outputs are bit-equal to those of the same call with a roomy, 256-byte aligned workspace,
and a call with `need - 1` bytes answers OQ_ERR_WORKSPACE and leaves every output as it was.  Every access stays inside the
test's own allocation.  All seven are run-to-run bit-stable (their own tests compare digests or exact bits), so no tolerance.

`oq_rtn_quantize_f32` with mse is the one whose refusal is asserted at another size than its query's: see `test_rtn_mse`."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD, PATTERN, SENTINEL = 256, 0xA5, 0x5C


@pytest.fixture(scope="module")
def L():
    from onnx_quantize_amd.hip import _lib
    _lib.load()
    return _lib


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


class Exact:
    """[guard | need bytes at `offset` behind a 256-byte boundary | guard] inside one device buffer filled with PATTERN"""

    def __init__(self, need, offset):
        self.buf = torch.full((need + 2 * GUARD + 512,), PATTERN, dtype=torch.uint8, device="cuda")
        self.start = (-self.buf.data_ptr()) % 256 + GUARD + offset
        self.need = need
        assert (self.buf.data_ptr() + self.start) % 256 == offset and self.start + need + GUARD <= self.buf.numel()

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + self.start)

    def guards_intact(self):
        return bool((self.buf[:self.start] == PATTERN).all()) and bool((self.buf[self.start + self.need:] == PATTERN).all())


def roomy(need):
    buf = torch.empty(need + 4096 + 256, dtype=torch.uint8, device="cuda")
    shift = (-buf.data_ptr()) % 256
    return buf, C.c_void_p(buf.data_ptr() + shift), need + 4096


def fresh(*specs):
    """output tensors filled with a sentinel byte"""
    return [torch.full(shape, SENTINEL, dtype=torch.uint8, device="cuda").view(dtype).reshape(shape_of) for shape, dtype, shape_of in specs]


def out(shape, dtype):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return ((n,), dtype, shape)


def run_exact(L, need, offset, call, n_inputs_checked=0):
    """call(workspace pointer, bytes) -> (status, [outputs]); the three assertions of the module docstring"""
    assert need > 0
    torch.cuda.synchronize()
    keep, wide, wide_bytes = roomy(need)
    st, want = call(wide, wide_bytes)
    assert st == 0, L.load().oq_last_error().decode()
    ex = Exact(need, offset)
    st, got = call(ex.ptr, need)
    torch.cuda.synchronize()
    assert st == 0, L.load().oq_last_error().decode()
    assert ex.guards_intact()
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g.view(torch.uint8), w.view(torch.uint8)), f"output {i} differs from the roomy call"
    short = Exact(need - 1, offset)
    st, untouched = call(short.ptr, need - 1)
    torch.cuda.synchronize()
    assert st == L.OQ_ERR_WORKSPACE, (st, L.load().oq_last_error().decode())
    assert short.guards_intact() and bool((short.buf == PATTERN).all())
    for i, t in enumerate(untouched[:len(untouched) - n_inputs_checked]):
        assert bool((t.view(torch.uint8) == SENTINEL).all()), f"output {i} touched by a refused call"
    return want, untouched


# ------------------------------------------------------------------------------------ oq_gptq_loop_f32
@pytest.mark.parametrize("block_size", [128, 256])      # > 128: the block's working copy exists
def test_gptq_loop(L, block_size):
    lib = L.load()
    K, N, g = 256, 64, 64
    W0 = torch.randn((K, N), device="cuda", generator=gen(1))
    U = torch.triu(torch.randn((K, K), device="cuda", generator=gen(2)) * 0.05) + torch.eye(K, device="cuda")
    s0 = torch.full((N,), 0.1, device="cuda")
    z0 = torch.full((N,), 8, dtype=torch.int32, device="cuda")
    need = lib.oq_gptq_loop_workspace_bytes(K, N, block_size)

    def call(ws, nbytes):
        W = W0.clone()
        q_int, q_deq, used_s, used_z = fresh(out((K, N), torch.uint8), out((K, N), torch.float32), out((K // g, N), torch.float32),
                                             out((K // g, N), torch.int32))
        st = lib.oq_gptq_loop_f32(ptr(W), K, N, ptr(U), L.OQ_UINT4, g, 0, 0, 1.0, 0, block_size, L.OQ_GPTQ_CORRECTED, 0, ptr(s0), ptr(z0), N,
                                  ptr(q_int), L.OQ_LAYOUT_KN, ptr(q_deq), ptr(used_s), ptr(used_z), ws, nbytes, None)
        return st, [q_int, q_deq, used_s, used_z, W]

    want, refused = run_exact(L, need, 8, call, n_inputs_checked=1)
    assert torch.equal(refused[-1], W0)                       # W is updated in place: a refused call leaves it
    assert int(want[0].max()) <= 15
    if block_size < K:                                        # a block that is all of W leaves W itself to its working copy
        assert not torch.equal(want[-1], W0)


# ------------------------------------------------------------------------------------ oq_hqq_optimize_f32
@pytest.mark.parametrize("per_round_launches", [0, 1])    # the one-pass route and the per-round loop
def test_hqq_optimize(L, per_round_launches):
    lib = L.load()
    K, N, g = 128, 64, 64
    rows = N * (K // g)
    W = torch.randn((K, N), device="cuda", generator=gen(3))
    scale = torch.rand((rows,), device="cuda", generator=gen(4)) * 0.2 + 0.1
    zp_in = torch.rand((rows,), device="cuda", generator=gen(5)) * 15.0
    need = lib.oq_hqq_workspace_bytes(K, N, g)

    def call(ws, nbytes):
        q, zp_out, rounds = fresh(out((K, N), torch.uint8), out((rows,), torch.float32), out((1,), torch.int32))
        st = lib.oq_hqq_optimize_f32(ptr(W), K, N, N, g, 0, ptr(scale), ptr(zp_in), 0.7, 10.0, 1.01, 20, 1, per_round_launches, ptr(q),
                                     L.OQ_LAYOUT_KN, ptr(zp_out), ptr(rounds), ws, nbytes, None)
        return st, [q, zp_out, rounds]

    want, _ = run_exact(L, need, 8, call)
    assert 1 <= int(want[2][0]) <= 20


# ------------------------------------------------------------------------------------ oq_rtn_quantize_f32, mse = 1
@pytest.mark.parametrize("strategy", ["group", "tensor"])
def test_rtn_mse(L, strategy):
    lib = L.load()
    K, N, g = 256, 64, 128
    code, gs, params = (L.OQ_GROUP, g, N * (K // g)) if strategy == "group" else (L.OQ_TENSOR, -1, 1)
    W = torch.randn((K, N), device="cuda", generator=gen(6))
    need = lib.oq_rtn_workspace_bytes(K, N, code, gs, 1)

    def call(ws, nbytes):
        q, scale, zp = fresh(out((K, N), torch.uint8), out((params,), torch.float32), out((params,), torch.uint8))
        st = lib.oq_rtn_quantize_f32(ptr(W), K, N, N, L.OQ_UINT4, code, gs, 0, 0, 1.0, 1, ptr(q), ptr(scale), ptr(zp), L.OQ_LAYOUT_KN, ws, nbytes, None)
        return st, [q, scale, zp]

    # oq_rtn_workspace_bytes(mse = 1) is the room of every route of oq_rtn_quantize_f32 PLUS the search's (test_mse_half_abi.py pins the
    # difference); with mse the call runs the search alone and has always been refused below the search's size only.  So the refusal
    # is asserted at that size, one byte short, and the exact-size run is made at both sizes.
    search = need - lib.oq_rtn_workspace_bytes(K, N, code, gs, 0)
    assert 0 < search <= need
    want, _ = run_exact(L, search, 8, call)
    assert int(want[0].max()) <= 15
    ex = Exact(need, 8)
    st, got = call(ex.ptr, need)
    torch.cuda.synchronize()
    assert st == 0 and ex.guards_intact() and all(torch.equal(a, b) for a, b in zip(got, want))


# ------------------------------------------------------------------------------------ oq_gptq_factor_f32
def test_gptq_factor(L):
    lib = L.load()
    K = 192                                                   # more than one diagonal block, no piece inverse
    X = torch.randn((4 * K, K), device="cuda", generator=gen(7))
    H = (X.t() @ X / (2 * K)).contiguous()
    need = lib.oq_gptq_factor_workspace_bytes(K)

    def call(ws, nbytes):
        U, info = fresh(out((K, K), torch.float32), out((1,), torch.int32))
        st = lib.oq_gptq_factor_f32(ptr(H), K, 0.01, ptr(U), ptr(info), 0, ws, nbytes, None)
        return st, [U, info]

    want, _ = run_exact(L, need, 8, call)
    assert int(want[1][0]) == 0 and bool(torch.isfinite(want[0]).all())


# ------------------------------------------------------------------------------------ oq_abs_stats_cols_many_h16
def test_abs_stats_cols_many(L):
    lib = L.load()
    T, widths = 64, (40, 72)
    xs = [torch.randn((T, k), device="cuda", generator=gen(8 + i)).to(torch.float16) for i, k in enumerate(widths)]

    def call(ws, nbytes):
        outs = [torch.zeros((k,), device="cuda") for k in widths for _ in range(2)]      # running values: start from zero
        host = np.asarray([(x.data_ptr(), T, k, k, outs[2 * i].data_ptr(), outs[2 * i + 1].data_ptr()) for i, (x, k) in enumerate(zip(xs, widths))],
                          dtype=np.int64)
        dev = torch.from_numpy(host).cuda()
        st = lib.oq_abs_stats_cols_many_h16(C.c_void_p(host.ctypes.data), ptr(dev), len(widths), L.OQ_W_F16, ws, nbytes, None)
        torch.cuda.synchronize()
        return st, outs

    host = np.asarray([(4096, T, k, k, 4096, 4096) for k in widths], dtype=np.int64)
    need = lib.oq_abs_stats_many_half_workspace_bytes(C.c_void_p(host.ctypes.data), len(widths))
    torch.cuda.synchronize()
    keep, wide, wide_bytes = roomy(need)
    st, want = call(wide, wide_bytes)
    assert st == 0
    ex = Exact(need, 8)
    st, got = call(ex.ptr, need)
    assert st == 0 and ex.guards_intact()
    for i, (x, k) in enumerate(zip(xs, widths)):
        assert torch.equal(got[2 * i], want[2 * i]) and torch.equal(got[2 * i + 1], want[2 * i + 1])
        assert torch.equal(want[2 * i + 1], x.float().abs().amax(dim=0))
    short = Exact(need - 1, 8)
    st, untouched = call(short.ptr, need - 1)
    assert st == L.OQ_ERR_WORKSPACE and bool((short.buf == PATTERN).all())
    assert all(bool((t == 0).all()) for t in untouched)


# ------------------------------------------------------------------------------------ oq_matmul_nbits, fp32 A, split K
def test_matmul_nbits(L):
    lib = L.load()
    M, K, N, g = 16, 512, 128, 32
    A = torch.randn((M, K), device="cuda", generator=gen(10))
    blob = torch.randint(0, 256, (N, K // g, g // 2), device="cuda", generator=gen(11), dtype=torch.uint8)
    scales = torch.rand((N, K // g), device="cuda", generator=gen(12)) * 0.02 + 0.001
    need = lib.oq_matmul_nbits_workspace_bytes(M, K, N, g, L.OQ_NBITS_F32)
    assert need == 2 * M * K * 2 + 256 + 8 * M * N * 4        # include/oq_hip_nbits.h: the pieces, the exponents, eight slabs

    def call(ws, nbytes):
        (Y,) = fresh(out((M, N), torch.float32))
        st = lib.oq_matmul_nbits(ptr(A), L.OQ_NBITS_F32, M, K, K, ptr(blob), 4, N, g, ptr(scales), L.OQ_NBITS_F32, None, None, 0, ptr(Y), N, ws,
                                 nbytes, None)
        return st, [Y]

    want, _ = run_exact(L, need, 0, call)
    assert bool(torch.isfinite(want[0]).all())


# ------------------------------------------------------------------------------------ oq_qlinear_matmul, split K
def test_qlinear_matmul(L):
    lib = L.load()
    M, K, N = 16, 512, 128
    A = torch.randint(0, 256, (M, K), device="cuda", generator=gen(13), dtype=torch.uint8)
    B = torch.randint(0, 256, (K, N), device="cuda", generator=gen(14), dtype=torch.uint8)
    a_zp = torch.tensor([3], dtype=torch.uint8, device="cuda")
    b_zp = torch.tensor([5], dtype=torch.uint8, device="cuda")
    need = lib.oq_qlinear_matmul_workspace_bytes(M, K, N)
    assert need == 256 + 8 * 512 + 8 * M * N * 4              # include/oq_hip_qlinear.h: row sums, eight slices of column sums, eight slabs

    def call(ws, nbytes):
        (Y,) = fresh(out((M, N), torch.int32))
        st = lib.oq_qlinear_matmul(ptr(A), L.OQ_QL_U8, M, K, K, None, ptr(a_zp), ptr(B), L.OQ_QL_U8, L.OQ_QL_KN, N, N, None, ptr(b_zp), 0, None, None,
                                   None, 0, L.OQ_QL_OUT_I32, ptr(Y), N, ws, nbytes, None)
        return st, [Y]

    want, _ = run_exact(L, need, 0, call)
    exact = (A.double() - 3) @ (B.double() - 5)               # |sum| < 2^26: exact in float64
    assert torch.equal(want[0].double(), exact)
