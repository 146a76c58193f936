"""What the QLinearMatMul / QGemm tests share (test_qlinear_matmul_abi.py, test_qlinear_matmul_gpu.py):

`plan`, `workspace`  the launch plan of csrc/qlinear_gemm.hip (the one of matmul_nbits.hip: nbits_cases.plan) and the header's R + C + S;
`Case`               two 8-bit operands on the device with their zero points, extremes forced, and the exact accumulator on the CPU;
`raw`                one call of `oq_qlinear_matmul` with every argument of the C ABI in reach (strides, C, the output code);
`restate`            the epilogue of include/oq_hip_qlinear.h in NumPy, every operand np.float32, in the stated order.
"""
import numpy as np
import torch

from nbits_cases import plan, r256

DT = {"u8": torch.uint8, "i8": torch.int8}
CODE = {torch.uint8: 0, torch.int8: 1}                                        # oq_ql_type
RANGE = {torch.uint8: (0, 255), torch.int8: (-128, 127)}
KN, NK = 0, 1                                                                 # oq_ql_layout
OUT_I32, OUT_F32, OUT_U8, OUT_I8 = range(4)                                   # oq_ql_out
OUT_DTYPE = {OUT_I32: torch.int32, OUT_F32: torch.float32, OUT_U8: torch.uint8, OUT_I8: torch.int8}
SIGNS = [("u8", "u8"), ("u8", "i8"), ("i8", "u8"), ("i8", "i8")]
LAYOUTS = {"KN": KN, "NK": NK}


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def workspace(M, K, N):
    """include/oq_hip_qlinear.h, `workspace`: R + C + S."""
    splits = plan(M, K, N).splits
    return r256(M * 4) + 8 * r256(N * 4) + (r256(splits * M * N * 4) if splits > 1 else 0)


def draw(g, shape, dtype, lo=None, hi=None):
    a, b = RANGE[dtype]
    lo, hi = (a if lo is None else max(a, lo)), (b if hi is None else min(b, hi))
    return torch.randint(lo, hi + 1, shape, device="cuda", generator=g, dtype=torch.int32).to(dtype)


class Case:
    """A [M, K] of `a_dt`, B of `b_dt` stored [K, N] (layout KN) or [N, K] (NK), random over the whole range of their types (so B is
    not symmetric in any sense), and zero points per `zp`:

      "lo"      a_zp at the bottom of A's type; b_zp per column, random, column 0 at the bottom and column N - 1 at the top
      "hi"      a_zp at the top; one b_zp, at the top
      "mid"     a_zp and one b_zp drawn inside the range
      "null"    no zero points;  "a_null" / "b_null": only that one missing, the other as in "lo"

    Extremes, in every 128-column tile: in output (0, n), n the tile's first column, the pairs (a, b) = (top, top), (top, bottom),
    (bottom, top) sit at k = 0, 1, 2 -- as many of them as K has room for.  `span`: A and B are drawn within +- span of their zero
    points instead (small accumulators for the epilogue tests; no extremes then)."""

    def __init__(self, g, M, K, N, a_dt, b_dt, layout, zp="lo", bias=False, span=None):
        self.M, self.K, self.N, self.layout = M, K, N, layout
        a_dt, b_dt = DT.get(a_dt, a_dt), DT.get(b_dt, b_dt)
        (a_lo, a_hi), (b_lo, b_hi) = RANGE[a_dt], RANGE[b_dt]
        a_zp = b_zp = None
        if zp in ("lo", "b_null"):
            a_zp = torch.tensor(a_lo, dtype=a_dt, device="cuda")
        if zp in ("lo", "a_null"):
            b_zp = draw(g, (N,), b_dt)
            b_zp[0] = b_lo
            b_zp[N - 1] = b_hi if N > 1 else b_lo
        if zp == "hi":
            a_zp, b_zp = torch.tensor(a_hi, dtype=a_dt, device="cuda"), torch.tensor(b_hi, dtype=b_dt, device="cuda")
        if zp == "mid":
            a_zp, b_zp = draw(g, (), a_dt, a_lo + 40, a_hi - 40), draw(g, (), b_dt, b_lo + 40, b_hi - 40)
        assert zp in ("lo", "hi", "mid", "null", "a_null", "b_null"), zp
        if span is None:
            a, b = draw(g, (M, K), a_dt), draw(g, (K, N), b_dt)
            first = torch.arange(0, N, 128, device="cuda")
            for k, (av, bv) in enumerate([(a_hi, b_hi), (a_hi, b_lo), (a_lo, b_hi)][:K]):
                a[0, k] = av
                b[k, first] = bv
        else:
            za = 0 if a_zp is None else int(a_zp)
            zb = 0 if b_zp is None else int(b_zp.reshape(-1)[0])
            assert b_zp is None or b_zp.numel() == 1
            a, b = draw(g, (M, K), a_dt, za - span, za + span), draw(g, (K, N), b_dt, zb - span, zb + span)
        self.a, self.a_zp, self.b_zp = a, a_zp, b_zp
        self.b = b.contiguous() if layout == KN else b.t().contiguous()         # as stored
        self.bias = torch.randint(-(1 << 20) - 1000, (1 << 20) + 1000, (N,), device="cuda", generator=g, dtype=torch.int32) if bias else None
        if bias:
            self.bias[0], self.bias[N - 1] = (1 << 20) + 999, -(1 << 20) - 999
        # the exact accumulator: every partial sum is an integer below 2^53, so the float64 product on the CPU IS the int64 product
        assert K * 255 * 255 + (1 << 21) < 1 << 31
        a64 = a.cpu().double() - (0.0 if a_zp is None else float(a_zp))
        b64 = b.cpu().double() - (0.0 if b_zp is None else b_zp.cpu().double().reshape(1, -1))
        acc = a64 @ b64
        if bias:
            acc = acc + self.bias.cpu().double()
        self.acc = acc.to(torch.int64)
        assert torch.equal(self.acc.double(), acc) and int(self.acc.abs().max()) < 1 << 31

    @property
    def trans_b(self):
        return self.layout == NK

    def plan(self):
        return plan(self.M, self.K, self.N)

    def want_i32(self):
        return self.acc.to(torch.int32)

    def matmul_integer(self, ops, a=None, b=None):
        return ops.matmul_integer(self.a if a is None else a, self.b if b is None else b, self.a_zp, self.b_zp, trans_b=self.trans_b)


def raw(lib, c, *, out=OUT_I32, a=None, lda=None, b=None, ldb=None, y=None, ldy=None, a_scale=None, b_scale=None, y_scale=None, y_zp=None,
        flags=0, a_code=None, b_code=None, layout=None, out_code=None):
    """`oq_qlinear_matmul` on the operands of Case `c`; `a`, `b`, `y` may be views with gaps (their leading dimension is passed along).
    Returns (status, y)."""
    a = c.a if a is None else a
    b = c.b if b is None else b
    lda = (a.stride(0) if a.shape[0] > 1 else a.shape[1]) if lda is None else lda
    ldb = (b.stride(0) if b.shape[0] > 1 else b.shape[1]) if ldb is None else ldb
    if y is None:
        y = torch.empty((c.M, c.N), dtype=OUT_DTYPE[out], device="cuda")
    ldy = (y.stride(0) if y.shape[0] > 1 else y.shape[1]) if ldy is None else ldy
    need = lib.oq_qlinear_matmul_workspace_bytes(c.M, c.K, c.N)
    assert need == workspace(c.M, c.K, c.N)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    per_column = int(any(t is not None and t.numel() == c.N and c.N > 1 for t in (b_scale, c.b_zp)))
    st = lib.oq_qlinear_matmul(a.data_ptr(), CODE[a.dtype] if a_code is None else a_code, c.M, c.K, lda, ptr(a_scale), ptr(c.a_zp), b.data_ptr(),
                               CODE[b.dtype] if b_code is None else b_code, c.layout if layout is None else layout, c.N, ldb, ptr(b_scale),
                               ptr(c.b_zp), per_column, ptr(c.bias), ptr(y_scale), ptr(y_zp), flags, out if out_code is None else out_code,
                               y.data_ptr(), ldy, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()                                 # `ws` is freed on return
    return st, y


def restate(acc, a_scale, b_scale, y_scale=None, y_zp=None, dtype=None):
    """The epilogue on exact accumulators, every operand np.float32, one rounding a step: np.float32(acc) * (a_s * b_s[n]), / y_s,
    np.rint, + zp, clip.  acc [M, N] int64 (NumPy); b_scale a scalar or [N].  Without y_scale: the fp32 value."""
    f = np.float32
    t = acc.astype(f) * (f(a_scale) * np.asarray(b_scale, f).reshape(1, -1))
    assert t.dtype == f
    if y_scale is None:
        return t
    lo, hi = RANGE[dtype]
    q = np.rint(t / f(y_scale)) + f(y_zp)
    assert q.dtype == f
    return np.clip(q, f(lo), f(hi)).astype(np.uint8 if dtype == torch.uint8 else np.int8)
