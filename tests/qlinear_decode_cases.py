"""What the tests of the QLinearMatMul / QGemm decode route share (test_qlinear_decode_abi.py, test_qlinear_decode_gpu.py):

`plan`, `workspace`  the launch plan of csrc/qlinear_decode_plan.hpp and the header's S, restated;
`raw_decode`         one call of `oq_qlinear_matmul_decode` with every argument of the C ABI in reach, in the shape of `qlinear_cases.raw`.
"""
from collections import namedtuple

KN, NK = 0, 1                                                                 # oq_ql_layout
MAX_ROWS, SLICE, SLICE_UNIT, COL_UNIT_NK, COLS_KN, WORKGROUPS = 16, 1024, 64, 16, 256, 512

Plan = namedtuple("Plan", "tier slice splits cols_per_block col_blocks grid slab_bytes last")


def ceil_div(a, b):
    return -(-a // b)


def r256(n):
    return (n + 255) // 256 * 256


def plan(M, K, N, layout):
    """include/oq_hip_qlinear_decode.h, `Plan`.  `last`: the k of the last slice."""
    tier = 1 if M <= 1 else 4 if M <= 4 else 8 if M <= 8 else 16
    if layout == NK:
        slice_ = SLICE
        splits = ceil_div(K, slice_)
        want = max(1, WORKGROUPS // splits)
        cols = ceil_div(ceil_div(N, want), COL_UNIT_NK) * COL_UNIT_NK
    else:
        cols = COLS_KN
        want = ceil_div(WORKGROUPS // 2 if tier >= 8 else WORKGROUPS, ceil_div(N, cols))
        slice_ = min(SLICE, ceil_div(ceil_div(K, want), SLICE_UNIT) * SLICE_UNIT)
        splits = ceil_div(K, slice_)
    col_blocks = ceil_div(N, cols)
    return Plan(tier, slice_, splits, cols, col_blocks, col_blocks * splits, splits * M * N * 4 if splits > 1 else 0, K - (splits - 1) * slice_)


def workspace(M, K, N, layout):
    """include/oq_hip_qlinear_decode.h, `workspace`: S."""
    return r256(plan(M, K, N, layout).slab_bytes)


def raw_decode(lib, c, *, out=0, a=None, lda=None, b=None, ldb=None, y=None, ldy=None, a_scale=None, b_scale=None, y_scale=None, y_zp=None,
               flags=0, a_code=None, b_code=None, layout=None, out_code=None, M=None):
    """`oq_qlinear_matmul_decode` on the operands of `qlinear_cases.Case` `c`; `a`, `b`, `y` may be views with gaps (their leading
    dimension is passed along); `M`: the row count handed over where it is not c's.  Returns (status, y)."""
    import torch
    from qlinear_cases import CODE, OUT_DTYPE
    a = c.a if a is None else a
    b = c.b if b is None else b
    lda = (a.stride(0) if a.shape[0] > 1 else a.shape[1]) if lda is None else lda
    ldb = (b.stride(0) if b.shape[0] > 1 else b.shape[1]) if ldb is None else ldb
    if y is None:
        y = torch.empty((c.M, c.N), dtype=OUT_DTYPE[out], device="cuda")
    ldy = (y.stride(0) if y.shape[0] > 1 else y.shape[1]) if ldy is None else ldy
    rows = c.M if M is None else M
    need = lib.oq_qlinear_matmul_decode_workspace_bytes(rows, c.K, c.N, c.layout)
    assert need == (workspace(rows, c.K, c.N, c.layout) if rows <= MAX_ROWS else 0)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    per_column = int(any(t is not None and t.numel() == c.N and c.N > 1 for t in (b_scale, c.b_zp)))
    st = lib.oq_qlinear_matmul_decode(a.data_ptr(), CODE[a.dtype] if a_code is None else a_code, rows, c.K, lda, ptr(a_scale), ptr(c.a_zp),
                                      b.data_ptr(), CODE[b.dtype] if b_code is None else b_code, c.layout if layout is None else layout, c.N, ldb,
                                      ptr(b_scale), ptr(c.b_zp), per_column, ptr(c.bias), ptr(y_scale), ptr(y_zp), flags,
                                      out if out_code is None else out_code, y.data_ptr(), ldy, ws.data_ptr() if need else None, need,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()                                 # `ws` is freed on return
    return st, y
