"""`ops.qdq_matmul_packed4` / `oq_qdq_matmul_packed4` (include/oq_hip_qdq_packed4.h, csrc/qdq_matmul_packed4.hip): the product of a
QDQ function from a 4-bit weight as packed nibbles [K, N / 2].  The reference everywhere is float64, as in test_qdq_matmul_gpu.py:
w64[k, n] = (q - zp[i]) * float64(scale[i]),  Y64 = A64 . w64 + bias64.  A case is a `qdq_cases.Case` narrowed to 4 bits."""
import itertools

import pytest
import torch

from nbits_cases import plan
from onnx_quantize_amd.hip import _lib, ops
from qdq_cases import ATYPE, DTYPES, GRANULARITY, Case, describe, gen

pytestmark = pytest.mark.gpu
UINT4, INT4 = 1, 0                                            # oq_qtype


def narrowed(*args, signed, **kw):
    """A `Case` whose W and zero points are its own shifted down to 4 bits (the forced ends of the 8-bit type stay the ends of the
    4-bit one), with w64 restated from them, and `packed`: W as the file stores it."""
    c = Case(*args, torch.int8 if signed else torch.uint8, **kw)
    c.w, c.zero_points = c.w >> 4, None if c.zero_points is None else c.zero_points >> 4
    blocks = c.K // c.group
    shape = (1, 1) if c.granularity == "tensor" else (c.N, blocks)
    zp = 0.0 if c.zero_points is None else c.zero_points.double().reshape(shape).expand(c.N, blocks)[:, :, None]
    s = c.scales.double().reshape(shape).expand(c.N, blocks)[:, :, None]
    c.w64 = ((c.w.t().double().reshape(c.N, blocks, c.group) - zp) * s).reshape(c.N, c.K).contiguous()
    c.signed = signed
    c.packed = ((c.w[:, 0::2] & 0x0F) | (c.w[:, 1::2] << 4)).view(torch.uint8)
    return c


def run(c, w=None):
    return ops.qdq_matmul_packed4(c.x, c.packed if w is None else w, c.scales, c.zero_points, n=c.N, signed=c.signed, group_size=c.group_size, bias=c.bias)


def raw(c, y, ldy, workspace, **over):
    a = dict(atype=ATYPE[c.dtype], K=c.K, wtype=INT4 if c.signed else UINT4, N=c.N, ldw=c.N // 2, group_size=c.group_size, workspace_bytes=workspace.numel())
    assert set(over) <= set(a), over
    a.update(over)
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    return _lib.load().oq_qdq_matmul_packed4(c.x.data_ptr(), a["atype"], c.M, a["K"], c.K, c.packed.data_ptr(), a["wtype"], a["N"], a["ldw"],
                                            GRANULARITY[c.granularity], a["group_size"], c.scales.data_ptr(), ATYPE[c.scales.dtype], ptr(c.zero_points),
                                            ptr(c.bias), y.data_ptr(), ldy, workspace.data_ptr(), a["workspace_bytes"],
                                            torch.cuda.current_stream().cuda_stream)


# |A| <= 4 integers, |q - zp| <= 15, scales in {1/8, 1/2, 1}, K <= 200: every partial sum is a multiple of 1/8 far below 2^24 / 8.
# M in {1, 33} (both row tiles) x K in {1, 3: fewer k than a thread's run of 4; 64; 67, 200: a run that straddles K, a second step}
# x N in {2, 6: no whole dword of a row; 8; 130: a second column tile with one byte; 136: ... with one whole dword}; per group
# g = 32 at K = 96 (two groups inside a step, a short last step) and g = 64 at K = 192.
SHAPES = [(1, 1, 2), (33, 3, 6), (1, 64, 8), (33, 67, 130), (1, 200, 136), (33, 200, 2), (1, 67, 6), (33, 64, 136), (1, 3, 130), (33, 1, 8),
          (33, 200, 130), (1, 64, 2)]
GROUPED = [(33, 96, 130, 32), (1, 96, 6, 32), (33, 192, 136, 64), (1, 192, 8, 64), (1, 96, 136, 32)]


@pytest.mark.parametrize("zero_points", [True, False], ids=["zp", "no zp"])
@pytest.mark.parametrize("signed", [False, True], ids=["uint4", "int4"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_integers_at_every_leg_of_the_staging(dt, signed, zero_points):
    g = gen(400)
    cases = [(M, K, N, gr) for (M, K, N), gr in itertools.product(SHAPES, ("tensor", "column"))] + GROUPED
    # K split across workgroups with a last split that holds fewer than its 64 k per step (at K <= 200 a split is one step)
    assert any(plan(M, K, N).splits > 1 and K < plan(M, K, N).splits * plan(M, K, N).steps_per_split * 64 for M, K, N, _ in cases)
    for i, (M, K, N, granularity) in enumerate(cases):
        c = narrowed(g, M, K, N, granularity, DTYPES[dt], signed=signed, zero_points=zero_points, bias=bool(i & 1), integer=True)
        wrong = run(c) != c.rounded(c.y64())
        assert not wrong.any(), ((M, K, N), granularity, describe(wrong, c.plan()))


@pytest.mark.parametrize("signed", [False, True], ids=["uint4", "int4"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_every_alignment_of_w_gives_the_same_bytes_and_the_gap_of_y_stays(dt, signed):
    """Base offsets 0 ... 3 with an odd ldw, aligned rows with a gap, the gaps full of garbage; ldy > N through the C ABI."""
    for (M, K, N), granularity in (((33, 200, 136), "column"), ((3, 192, 22), 64), ((17, 67, 130), "tensor")):
        c = narrowed(gen(11), M, K, N, granularity, DTYPES[dt], signed=signed, integer=True)
        want = run(c)
        assert torch.equal(want, c.rounded(c.y64()))
        half = N // 2
        for offset, ldw in itertools.chain(((o, half + (1 - half) % 4) for o in range(4)), ((0, half + (-half) % 4 + 8),)):
            flat = torch.randint(0, 256, (offset + K * ldw + 3,), device="cuda", generator=gen(offset), dtype=torch.int32).to(torch.uint8)
            w = flat[offset:offset + K * ldw].reshape(K, ldw)[:, :half]
            w.copy_(c.packed)
            assert w.data_ptr() % 4 == offset and w.stride(0) == ldw
            wrong = run(c, w) != want
            assert not wrong.any(), (offset, ldw, describe(wrong, c.plan()))
        y = torch.full((M, N + 5), -77.0, device="cuda", dtype=c.dtype)
        ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
        assert raw(c, y, N + 5, ws) == 0, _lib.load().oq_last_error()
        assert torch.equal(y[:, :N], want) and (y[:, N:] == -77.0).all()


@pytest.mark.parametrize("shape", [(70, 1024, 260), (3, 4096, 64)], ids=str)
@pytest.mark.parametrize("granularity", ["tensor", "column", 128])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_random_data_stays_inside_the_derived_bound(dt, granularity, shape):
    """Case.bound() with blocks = K / g, or 1: the operands are a subset of the byte route's, which gives the same bytes."""
    c = narrowed(gen(21), *shape, granularity, DTYPES[dt], signed=granularity == "column")
    y, y64 = run(c), c.y64()
    excess = ((y.to(torch.float64) - y64).abs() - c.bound()).max().item()
    print(f"{dt} {granularity} {shape}: max(|err| - bound) = {excess:.3e}")
    assert y.dtype == c.dtype and y.shape == shape[::2] and excess <= 0.0
    assert torch.equal(y.view(torch.uint8), c.run(ops).view(torch.uint8))


def test_refusals_leave_y_untouched_and_the_op_raises_by_name():
    c = narrowed(gen(61), 8, 256, 16, 32, torch.float16, signed=False, bias=False, integer=True)      # K in four steps: slabs, so a workspace
    y = torch.full((8, 16), -77.0, device="cuda", dtype=torch.float16)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    last_error = _lib.load().oq_last_error
    for kw, status, word in ((dict(N=15), -2, "N = 15 is odd"), (dict(wtype=3), -1, "wtype"), (dict(group_size=48), -2, "group_size = 48"),
                             (dict(K=96, group_size=64), -2, "no multiple of group_size"), (dict(workspace_bytes=64), -3, "workspace"),
                             (dict(ldw=7), -1, "ldw=7")):
        assert raw(c, y, 16, ws, **kw) == status, (kw, last_error())
        assert word in last_error().decode(), (kw, last_error())
    torch.cuda.synchronize()
    assert (y == -77.0).all()
    assert raw(c, y, 16, ws) == 0
    assert torch.equal(y, c.rounded(c.y64()))
    with pytest.raises(NotImplementedError, match="N = 15"):
        ops.qdq_matmul_packed4(c.x, c.packed, c.scales, c.zero_points, n=15, signed=False, group_size=32)
    with pytest.raises(NotImplementedError, match="zero point of torch.uint8"):
        ops.qdq_matmul_packed4(c.x, c.packed, c.scales, c.zero_points, n=16, signed=True, group_size=32)
