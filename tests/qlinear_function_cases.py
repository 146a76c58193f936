"""What the tests of the QLinear function route share (test_qlinear_function_abi.py, test_qlinear_function_gpu.py):

`workspace`, `decode_workspace`   the header's Q + R + C + S and S, restated;
`quantize_np`                     the quantizer of include/oq_hip_qlinear_function.h in NumPy: np.float32 divide, np.rint, + zp, clip,
                                  NaN -> the bottom of the type;
`draw_x`, `EDGES`, `plant`        fp32 activations around the levels of a type, ties, and the hostile values;
`FCase`                           a `qlinear_cases.Case` with an fp32 X in front: the exact accumulator of the QUANTIZED X on the CPU
                                  and the expected Y -- `qlinear_cases.restate`, then (q - zp) * y_scale in np.float32;
`raw_function`                    one call of `oq_qlinear_function` / `oq_qlinear_function_decode` with every argument in reach.
"""
import numpy as np
import torch

import qlinear_cases
import qlinear_decode_cases
from qlinear_cases import CODE, DT, KN, RANGE, Case, r256, restate

F = np.float32
NP_OF = {torch.uint8: np.uint8, torch.int8: np.int8}


def r16(n):
    return (n + 15) // 16 * 16


def workspace(M, K, N):
    """include/oq_hip_qlinear_function.h, `workspace`: Q ahead of R + C + S."""
    return r256(M * r16(K)) + qlinear_cases.workspace(M, K, N)


def decode_workspace(M, K, N, layout):
    return qlinear_decode_cases.workspace(M, K, N, layout)


def quantize_np(x, scale, zp, dtype):
    """q = sat(rint(x / scale) + zp), every step one np.float32 operation; a NaN gives the bottom of the type.  int64 [M, K]."""
    lo, hi = RANGE[dtype]
    with np.errstate(all="ignore"):
        q = np.rint(np.asarray(x, F) / F(scale)) + F(zp)
    assert q.dtype == F
    return np.where(np.isnan(q), F(lo), np.clip(q, F(lo), F(hi))).astype(np.int64)


def draw_x(rng, q0, zp, scale, ties=False):
    """x = (q0 - zp + u) * scale, u uniform in (-0.49, 0.49); `ties`: u = +-0.5 in every fourth position (exact for a scale 2^-k), so
    that even and odd q0 both meet a tie from either side."""
    u = rng.uniform(-0.49, 0.49, q0.shape)
    if ties:
        flat = u.reshape(-1)
        flat[0::8], flat[4::8] = 0.5, -0.5
    return ((q0.astype(np.float64) - zp + u) * scale).astype(F)


def edges(zp, scale, dtype):
    """One and 1000 levels beyond both ends, +-inf, +-0, a subnormal, 3.39e38 (against a scale below 1: the quotient overflows), NaN."""
    lo, hi = RANGE[dtype]
    return np.array([(lo - 1 - zp) * scale, (lo - 1000 - zp) * scale, (hi + 1 - zp) * scale, (hi + 1000 - zp) * scale, np.inf, -np.inf, 0.0, -0.0,
                     1e-40, 3.39e38, -3.39e38, np.nan], dtype=F)


def plant(x, values):
    """Value i into row i % M at the first, a middle and the last position and at the first position of the last 16-chunk (partial
    where K is no multiple of 16); rows are taken in turn, a later value overwrites an earlier one where M is small."""
    M, K = x.shape
    for i, v in enumerate(values):
        for k in (0, K // 2, K - 1, 16 * ((K - 1) // 16)):
            x[(i + k) % M, k] = v
    return x


class FCase:
    """A `Case` (B, the zero points, the bias, the layout) behind an fp32 X [M, K] whose quantization to `a_dt` covers the whole type.
    `scale`: x_scale; `ties`: plant ties (use a power of two); `hostile`: plant `edges`; `per_column`: b_scale per column."""

    def __init__(self, g, seed, M, K, N, a_dt, b_dt, layout, zp="lo", bias=False, scale=0.0123, ties=False, hostile=False, per_column=False,
                 y_dt=torch.uint8, y_zp=None):
        self.c = c = Case(g, M, K, N, a_dt, b_dt, layout, zp=zp, bias=bias)
        self.M, self.K, self.N, self.layout = M, K, N, layout
        self.a_dt, self.y_dt = DT.get(a_dt, a_dt), y_dt
        rng = np.random.default_rng(seed)
        za = 0 if c.a_zp is None else int(c.a_zp)
        x = draw_x(rng, c.a.cpu().numpy().astype(np.int64), za, scale, ties)
        if hostile:
            plant(x, edges(za, scale, self.a_dt))
        self.x_np, self.x = x, torch.from_numpy(x).cuda()
        self.a_scale = torch.tensor(scale, dtype=torch.float32, device="cuda")
        b_s = rng.uniform(0.008, 0.012, N).astype(F) if per_column and N > 1 else np.array([0.01], F)
        self.b_scale = torch.from_numpy(b_s).cuda() if per_column and N > 1 else torch.tensor(float(b_s[0]), dtype=torch.float32, device="cuda")
        # the exact accumulator of the quantized X, as Case makes its own: float64 products of integers below 2^53
        q = quantize_np(x, scale, za, self.a_dt)
        self.q = q
        b = c.b.cpu().double() if layout == KN else c.b.cpu().double().t()
        b64 = b - (0.0 if c.b_zp is None else c.b_zp.cpu().double().reshape(1, -1))
        acc = torch.from_numpy((q - za).astype(np.float64)) @ b64
        if bias:
            acc = acc + c.bias.cpu().double()
        self.acc = acc.to(torch.int64).numpy()
        assert np.array_equal(self.acc.astype(np.float64), acc.numpy()) and np.abs(self.acc).max() < 1 << 31
        # an output scale that spreads the products over about +-100 levels, not a power of two
        spread = float(np.abs(self.acc.astype(np.float64) * scale * float(b_s.mean())).max())
        y_s = F(max(spread, 1e-3) / 100.0 * 1.0137)
        lo, hi = RANGE[y_dt]
        self.y_zp_value = (lo + hi + 1) // 2 if y_zp is None else y_zp
        self.y_scale = torch.tensor(float(y_s), dtype=torch.float32, device="cuda")
        self.y_zp = torch.tensor(self.y_zp_value, dtype=y_dt, device="cuda")
        qy = restate(self.acc, scale, b_s, y_s, self.y_zp_value, y_dt)
        self.qy = qy
        self.want = (qy.astype(F) - F(self.y_zp_value)) * F(y_s)
        assert self.want.dtype == F

    def args(self, x=None):
        c = self.c
        return (self.x if x is None else x, self.a_scale, c.a_zp, c.b, self.b_scale, c.b_zp, self.y_scale, self.y_zp)

    def call(self, fn, x=None):
        return fn(*self.args(x), bias=self.c.bias, trans_b=self.c.trans_b)


def same_bytes(got, want):
    """fp32 results equal as bytes (a tensor on the device against a NumPy array or another tensor)."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else want
    return got.shape == want.shape and got.dtype == want.dtype == F and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def raw_function(lib, f, *, decode=False, x=None, lda=None, y=None, ldy=None, flags=0, a_code=None, b_code=None, layout=None, y_code=None, M=None,
                 workspace_bytes=None):
    """`oq_qlinear_function` (`decode`: `oq_qlinear_function_decode`) on FCase `f`; `x` and `y` may be views with gaps.  (status, y)."""
    c = f.c
    x = f.x if x is None else x
    lda = (x.stride(0) if x.shape[0] > 1 else x.shape[1]) if lda is None else lda
    if y is None:
        y = torch.empty((f.M, f.N), dtype=torch.float32, device="cuda")
    ldy = (y.stride(0) if y.shape[0] > 1 else y.shape[1]) if ldy is None else ldy
    ldb = c.b.stride(0) if c.b.shape[0] > 1 else c.b.shape[1]
    rows = f.M if M is None else M
    if decode:
        need = lib.oq_qlinear_function_decode_workspace_bytes(rows, f.K, f.N, f.layout)
        assert need == (decode_workspace(rows, f.K, f.N, f.layout) if rows <= 16 else 0)
    else:
        need = lib.oq_qlinear_function_workspace_bytes(rows, f.K, f.N)
        assert need == workspace(rows, f.K, f.N)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    per_column = int(any(t is not None and t.numel() == f.N and f.N > 1 for t in (f.b_scale, c.b_zp)))
    wide = lambda t: t.reshape(1).expand(f.N).contiguous() if per_column and t is not None and t.numel() == 1 else t      # noqa: E731
    b_scale, b_zp = wide(f.b_scale), wide(c.b_zp)      # the library takes one flag for both
    entry = lib.oq_qlinear_function_decode if decode else lib.oq_qlinear_function
    st = entry(x.data_ptr(), CODE[f.a_dt] if a_code is None else a_code, rows, f.K, lda, ptr(f.a_scale), ptr(c.a_zp), c.b.data_ptr(),
               CODE[c.b.dtype] if b_code is None else b_code, f.layout if layout is None else layout, f.N, ldb, ptr(b_scale), ptr(b_zp),
               per_column, ptr(c.bias), ptr(f.y_scale), ptr(f.y_zp), flags, CODE[f.y_dt] if y_code is None else y_code, y.data_ptr(), ldy,
               ws.data_ptr() if need else None, need if workspace_bytes is None else workspace_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()                                 # `ws` is freed on return
    return st, y
