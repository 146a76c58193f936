"""`oq_gptq_factor_f32`, `oq_gptq_factor_batched_f32` and `oq_gptq_prepare_f32` against closed forms, bit for bit
(tests/gptq_factor_cases.py has the argument and the recipes, tests/test_gptq_factor_cases.py checks them on the host).

On the exact cases every number the chain of csrc/factor.hip forms is a small dyadic rational, so U does not depend on the blocking,
the summation order or the leg of a product (register loops, LDS products, the fp32 GEMM on either load arm, the fp16 pieces): the
kernels owe the closed form's bits, `info` its documented value, and a failure names the launch that wrote the wrong block
(`describe`).  There is no tolerance in this file.  One thing the closed form does not define is the sign of a zero: the kernels
negate sums (X21 = -(X22 S)), so a structural zero of U may come out as -0.0; `+ 0.0` maps it to +0.0 before the bits are compared,
and changes no other value.  Comparisons between two runs of the kernels are on the raw bytes."""
import numpy as np
import pytest
import torch

import gptq_factor_cases as F

pytestmark = pytest.mark.gpu

PIVOT_K = 388
PIVOTS = (0, 31, 32, 127, 128, 384, 387)
KINDS = ("zero", "negative", "nan")
INVALID, WORKSPACE = -1, -3
METHOD = {"auto": 0, "f32": 1}
SENTINEL = np.float32(-12345.0)


@pytest.fixture(scope="module")
def ops():
    from onnx_quantize_amd.hip import ops
    return ops


@pytest.fixture(scope="module")
def lib():
    from onnx_quantize_amd.hip import _lib
    return _lib.load()


def bits(x):
    return (np.ascontiguousarray(x, dtype=np.float32) + np.float32(0.0)).view(np.uint32)


def assert_factor(case, u, info, what):
    K = case.K
    assert int(info) == case.info, f"{case.name} [{what}]: info {int(info)}, owed {case.info}"
    wrong = bits(u) != bits(case.u)
    if wrong.any():
        r, c = np.argwhere(wrong)[0]
        pytest.fail(f"{case.name} [{what}]: " + F.describe(K, wrong) + f"; first at U[{r}][{c}] = {u[r, c]!r}, owed {case.u[r, c]!r}")


def factor(ops, case, method="auto"):
    u, info = ops.gptq_factor(torch.from_numpy(case.h).cuda(), case.percdamp, method)
    torch.cuda.synchronize()
    return u.cpu().numpy(), info.cpu().numpy()[0]


# ------------------------------------------------------------------------------------ 1. exact U
@pytest.mark.parametrize("K,method", [(K, m) for K in F.WIDTHS for m in F.methods_of(K)])
def test_exact_u(ops, K, method):
    """Every width of the table in tests/test_gptq_factor_cases.py::test_legs_restate_the_table; from 1536 on under both methods.
    Which leg ran is `legs()`'s statement: both are exact, their bits agree."""
    case = F.width_case(K)
    assert_factor(case, *factor(ops, case, method), method)


@pytest.mark.parametrize("K", F.DAMPED)
def test_exact_u_damped(ops, K):
    """H = H' - d I with the fp32 percdamp whose product with the mean of the diagonal is d exactly"""
    case = F.width_case(K, damped=True)
    assert case.percdamp > 0
    assert_factor(case, *factor(ops, case), "damped")


# ------------------------------------------------------------------------------------ 2. pivot verdicts
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("j", PIVOTS)
def test_pivot_verdict(ops, j, kind):
    """info = j + 1, the 1-based index of the first non-positive pivot in reversed index space, and U = I: in the first and last
    lane of a 32-sub-block, across the sub-block and the 128-block edge, and in the ragged block (n = 4, so + bad <= n)."""
    case = F.pivot_case(F.width_case(PIVOT_K), j, kind)
    assert_factor(case, *factor(ops, case), kind)


def test_first_pivot_wins(ops):
    """two spoiled pivots in different blocks: the later block finds `info` set and leaves it"""
    case = F.pivot_case(F.width_case(PIVOT_K), [(40, "zero"), (300, "nan")])
    assert case.info == 41
    assert_factor(case, *factor(ops, case), "two pivots")
    case = F.pivot_case(F.width_case(PIVOT_K), [(386, "negative"), (130, "nan")])
    assert case.info == 131
    assert_factor(case, *factor(ops, case), "two pivots, the later one given first")


def test_dead_channel(ops):
    """a zero diagonal entry at i with percdamp = 0: pivot K - 1 - i is zero without the fix, and the exact U with it"""
    i = 100
    case = F.width_case(PIVOT_K, dead=(i,))
    h = torch.from_numpy(case.h).cuda()
    u, info = ops.gptq_factor(h, 0.0)
    torch.cuda.synchronize()
    unfixed = F.Case(**{**case.__dict__, "u": np.eye(PIVOT_K, dtype=np.float32), "info": PIVOT_K - i})
    assert_factor(unfixed, u.cpu().numpy(), info.cpu().numpy()[0], "fix_dead = 0")
    u, info = ops.gptq_factor_batched(h[None], 0.0, fix_dead=False)
    torch.cuda.synchronize()
    assert_factor(unfixed, u.cpu().numpy()[0], info.cpu().numpy()[0], "batched, fix_dead = 0")
    u, info = ops.gptq_factor_batched(h[None], 0.0, fix_dead=True)
    torch.cuda.synchronize()
    assert_factor(case, u.cpu().numpy()[0], info.cpu().numpy()[0], "batched, fix_dead = 1")


# ------------------------------------------------------------------------------------ 3. batched, strides above K K
@pytest.mark.parametrize("K,count", [(388, 3), (640, 3), (1536, 2)])
def test_batched_strides(lib, K, count):
    """h_stride = u_stride = K K + 36: the gaps of H hold NaN, those of U a sentinel that must survive; every member is another
    matrix, member 1 has a spoiled pivot and owes I with its own info while its neighbours owe their exact U."""
    stride = K * K + 36
    cases = [F.width_case(K, seed=10 + m) for m in range(count)]
    cases[1] = F.pivot_case(cases[1], K - 3, "zero")
    h = np.full(count * stride, np.nan, dtype=np.float32)
    for m, c in enumerate(cases):
        h[m * stride:m * stride + K * K] = c.h.reshape(-1)
    hd = torch.from_numpy(h).cuda()
    ud = torch.full((count * stride,), float(SENTINEL), dtype=torch.float32, device="cuda")
    info = torch.full((count,), -7, dtype=torch.int32, device="cuda")
    need = lib.oq_gptq_factor_batched_workspace_bytes(K, count)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = lib.oq_gptq_factor_batched_f32(hd.data_ptr(), K, stride, count, 0.0, 0, ud.data_ptr(), stride, info.data_ptr(), METHOD["auto"],
                                        ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    assert st == 0
    u, got_info = ud.cpu().numpy(), info.cpu().numpy()
    assert np.array_equal(hd.cpu().numpy().view(np.uint32), h.view(np.uint32)), "H is read only"
    for m, c in enumerate(cases):
        gap = u[m * stride + K * K:(m + 1) * stride]
        assert np.array_equal(gap, np.full(36, SENTINEL)), f"member {m}: the gap behind U was written"
        assert_factor(c, u[m * stride:m * stride + K * K].reshape(K, K), got_info[m], f"member {m} of {count}")


# ------------------------------------------------------------------------------------ 4. workspace history
def factor_in(lib, case, ws, method="auto"):
    K = case.K
    need = lib.oq_gptq_factor_workspace_bytes(K)
    assert ws.numel() >= need
    h = torch.from_numpy(case.h).cuda()
    u = torch.empty((K, K), dtype=torch.float32, device="cuda")
    info = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    st = lib.oq_gptq_factor_f32(h.data_ptr(), K, case.percdamp, u.data_ptr(), info.data_ptr(), METHOD[method], ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    assert st == 0
    return u.cpu().numpy(), info.cpu().numpy()[0]


@pytest.mark.parametrize("K", (388, 1100, 1664, 2176))
def test_workspace_of_ff_bytes(lib, K):
    """the caller's workspace holds 0xFF bytes (NaN wherever a float is read) before the call: X / Y are cleared, S is written before it
    is read, Dinv and the operand pieces are zero-padded by the call itself -- the same bytes as from a zeroed workspace"""
    case = F.width_case(K)
    need = lib.oq_gptq_factor_workspace_bytes(K)
    dirty = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    u, info = factor_in(lib, case, dirty)
    assert_factor(case, u, info, "0xFF workspace")
    fresh, info0 = factor_in(lib, case, torch.zeros(need, dtype=torch.uint8, device="cuda"))
    assert info0 == info and np.array_equal(u.view(np.uint32), fresh.view(np.uint32))


def test_workspace_reused_across_widths(lib):
    """K = 640 in the workspace a K = 1100 call has just used (other strides, other block counts, a smaller Dinv)"""
    big, small = F.width_case(1100), F.width_case(640)
    ws = torch.full((lib.oq_gptq_factor_workspace_bytes(1100),), 0xFF, dtype=torch.uint8, device="cuda")
    assert_factor(big, *factor_in(lib, big, ws), "first call")
    u, info = factor_in(lib, small, ws)
    assert_factor(small, u, info, "second call in the same workspace")
    fresh, info0 = factor_in(lib, small, torch.zeros(lib.oq_gptq_factor_workspace_bytes(640), dtype=torch.uint8, device="cuda"))
    assert info0 == info and np.array_equal(u.view(np.uint32), fresh.view(np.uint32))


# ------------------------------------------------------------------------------------ 5. oq_gptq_prepare_f32
def prepare_data(K, N, seed):
    """W [K, N], symmetric H [K, K] whose diagonal has many ties, dead channels (+0.0 and one -0.0) among them and a few negative
    entries; every element of W and H is distinct enough to tell rows and columns apart"""
    rng = np.random.default_rng([seed, K, N])
    w = rng.standard_normal((K, N)).astype(np.float32)
    h = rng.standard_normal((K, K)).astype(np.float32)
    h = (h + h.T).astype(np.float32)
    diag = rng.choice(np.array([0.0, 0.5, 0.5, 1.0, 1.0, 1.0, 2.0, 3.0, -1.0], dtype=np.float32), size=K)
    if K > 2:
        diag[K // 2] = np.float32(-0.0)
        diag[K - 1] = 1.0                   # ties with the value the dead channels get
        diag[0] = 0.0
    h[np.arange(K), np.arange(K)] = diag
    return w, h


def prepare_expected(w, h, actorder):
    w, h = w.copy(), h.copy()
    dead = np.diagonal(h) == 0
    w[dead, :] = 0.0
    h[dead, dead] = 1.0
    if not actorder:
        return w, h, None
    perm = np.argsort(np.diagonal(h), kind="stable")[::-1]
    return w[perm], h[perm][:, perm], perm.astype(np.int32)


def run_prepare(lib, w, h, actorder, perm_null=False, short=0):
    K, N = w.shape
    wd, hd = torch.from_numpy(w).cuda(), torch.from_numpy(h).cuda()
    perm = torch.full((K,), -1, dtype=torch.int32, device="cuda")
    need = lib.oq_gptq_prepare_workspace_bytes(K, N, actorder)
    ws = torch.full((max(need, 256),), 0xFF, dtype=torch.uint8, device="cuda")
    st = lib.oq_gptq_prepare_f32(wd.data_ptr(), K, N, hd.data_ptr(), actorder, None if perm_null else perm.data_ptr(), ws.data_ptr(),
                                 need - short, None)
    torch.cuda.synchronize()
    return st, wd.cpu().numpy(), hd.cpu().numpy(), perm.cpu().numpy()


@pytest.mark.parametrize("actorder", (0, 1))
@pytest.mark.parametrize("N", (1, 255, 257))
@pytest.mark.parametrize("K", (1, 255, 256, 257))
def test_prepare(lib, K, N, actorder):
    w, h = prepare_data(K, N, 5)
    if K > 2:
        d = np.diagonal(h)
        assert (d == 0).sum() >= 2 and np.signbit(d[K // 2]) and len(np.unique(d)) < K // 8
    st, gw, gh, gperm = run_prepare(lib, w, h, actorder)
    assert st == 0
    ew, eh, eperm = prepare_expected(w, h, actorder)
    dead = np.diagonal(h) == 0
    if actorder:
        assert np.array_equal(gperm, eperm), f"perm differs first at rank {np.argwhere(gperm != eperm)[0][0]}"
        dead = dead[eperm]
    else:
        assert (gperm == -1).all(), "perm_out was written without actorder"
    assert not gw[dead].any() and (gh[dead, dead] == 1.0).all(), "dead channels"
    assert np.array_equal(gw.view(np.uint32), ew.view(np.uint32)), "W"
    assert np.array_equal(gh.view(np.uint32), eh.view(np.uint32)), "H"


@pytest.mark.parametrize("K,N", [(255, 257), (257, 1)])
def test_prepare_refusals_leave_w_and_h(lib, K, N):
    """actorder with a null perm_out, or a workspace one byte short: the status, and W and H byte for byte as they were -- dead
    channels included, whose fix would otherwise be the first launch"""
    w, h = prepare_data(K, N, 6)
    for kw, status in ((dict(perm_null=True), INVALID), (dict(short=1), WORKSPACE)):
        st, gw, gh, gperm = run_prepare(lib, w, h, 1, **kw)
        assert st == status, kw
        assert np.array_equal(gw.view(np.uint32), w.view(np.uint32)) and np.array_equal(gh.view(np.uint32), h.view(np.uint32)), kw
        assert (gperm == -1).all()
