"""What the tests of the QDQ function route share (test_qdq_function_abi.py, test_qdq_function_gpu.py, scripts/time_qdq_function.py):

`workspace`          the header's Q + R + C + S + P + PX + PO, restated;
`dyn_params`, `dyn_q`  DynamicQuantizeLinear as include/oq_hip_qdq_function.h states it, np.float32 operation by operation;
`restate`            the whole arithmetic block of the header in NumPy: np.float32 steps in the stated order, the product of the
                     integers in float64 (every partial sum is an integer below 2^53: it IS the int64 product);
`QCase`              operands on the device for one call, every mode and zero-point form, and the expected Y;
`raw`                one call of `oq_qdq_function` with every argument in reach.
"""
import numpy as np
import torch

import qlinear_cases
from nbits_cases import plan
from qlinear_cases import CODE, DT, RANGE, r256
from qlinear_function_cases import F, quantize_np, r16

NONE, STATIC, DYNAMIC = 0, 1, 2                      # oq_qdq_mode
MODE = {None: NONE, "static": STATIC, "dynamic": DYNAMIC}
F32, F16, BF16 = 0, 1, 2                             # oq_nbits_type
INT4, UINT4, INT8, UINT8 = 0, 1, 2, 3                # oq_qtype
WTYPE = {torch.uint8: UINT8, torch.int8: INT8}
TENSOR, CHANNEL, GROUP = 0, 1, 2                     # oq_strategy
COMBOS = [("static", None), ("static", "static"), ("static", "dynamic"), ("dynamic", None), ("dynamic", "static"), ("dynamic", "dynamic")]


def workspace(M, K, N, x_mode, out_mode):
    """include/oq_hip_qdq_function.h, `workspace`."""
    pl = plan(M, K, N)
    total = r256(M * r16(K)) + qlinear_cases.workspace(M, K, N)
    if x_mode == DYNAMIC:
        total += 256 + r256(8 * min(-(-M // 4), 2048))
    if out_mode == DYNAMIC:
        total += r256(8 * (pl.tiles if pl.splits == 1 else -(-M * N // 256)))
    return total


def dyn_params(t):
    """(safe, scale, zp) of a tensor; np.min / np.max propagate NaN."""
    with np.errstate(all="ignore"):
        lo, hi = np.minimum(np.min(t), F(0)), np.maximum(np.max(t), F(0))
        scale = F(hi - lo) / F(255)
        safe = F(1) if scale == 0 else scale
        zp = np.rint(np.clip(-lo / safe, F(0), F(255)))
    assert all(np.asarray(v).dtype == F for v in (lo, hi, scale, safe, zp))
    return safe, scale, zp


def dyn_q(t, safe, zp):
    q = np.clip(np.rint(t / safe) + zp, F(0), F(255))
    assert q.dtype == F
    return q


def restate(x, x_mode, x_dt, x_scale, x_zp, w, w_scale, w_zp, bias, out_mode, out_dt, out_scale, out_zp):
    """x [M, K] fp32, w [K, N] integers, w_scale / w_zp scalars or [N], bias None or (B int [N], b_scale, b_zp).  (Y, S, v)."""
    x = np.asarray(x, F)
    if x_mode == "dynamic":
        safe, xs, zp = dyn_params(x)
        if np.isnan(xs):
            nan = np.full((x.shape[0], w.shape[1]), np.nan, F)
            return nan, None, nan
        q, zx = dyn_q(x, safe, zp).astype(np.int64), int(zp)
    else:
        xs, zx = F(x_scale), 0 if x_zp is None else int(x_zp)
        q = quantize_np(x, xs, zx, x_dt)
    wz = np.zeros(1, np.int64) if w_zp is None else np.asarray(w_zp, np.int64).reshape(-1)
    prod = (q - zx).astype(np.float64) @ (np.asarray(w, np.int64) - wz.reshape(1, -1)).astype(np.float64)
    S = prod.astype(np.int64)
    assert np.array_equal(S.astype(np.float64), prod) and np.abs(S).max(initial=0) < 1 << 31
    v = S.astype(F) * (xs * np.asarray(w_scale, F).reshape(1, -1))
    if bias is not None:
        B, b_scale, b_zp = bias
        v = v + ((np.asarray(B, np.int64).astype(F) - F(0 if b_zp is None else int(b_zp))) * F(b_scale)).reshape(1, -1)
    assert v.dtype == F
    if out_mode is None:
        return v, S, v
    if out_mode == "static":
        lo, hi = RANGE[out_dt]
        zo = F(0 if out_zp is None else int(out_zp))
        q = np.clip(np.rint(v / F(out_scale)) + zo, F(lo), F(hi))
        y = (q - zo) * F(out_scale)
    else:
        safe, scale, zp = dyn_params(v)
        y = (dyn_q(v, safe, zp) - zp) * scale
    assert y.dtype == F
    return y, S, v


def zero_point(g, form, dtype, n=1):
    """"lo" / "hi": that end of the type (per column: random with column 0 at the bottom and the last at the top); "mid"; None."""
    lo, hi = RANGE[dtype]
    if form is None:
        return None
    if n > 1:
        z = qlinear_cases.draw(g, (n,), dtype)
        z[0], z[n - 1] = (lo, hi) if form == "lo" else (hi, lo)
        return z
    return torch.tensor({"lo": lo, "hi": hi, "mid": (lo + hi + 1) // 2 + 3}[form], dtype=dtype, device="cuda")


class QCase:
    """One call: X around the levels of its type (static) or standard normal (dynamic) unless `x` is given, W over its whole type
    unless `w` is given, the parameters per `*_zp` ("lo", "hi", "mid", None) and `per_column`, a Gemm's bias triple with `gemm`."""

    def __init__(self, seed, M, K, N, x_mode, out_mode, x_dt="u8", w_dt="i8", x_zp="mid", w_zp="lo", out_zp="mid", out_dt="u8", gemm=False,
                 per_column=True, x=None, w=None, x_scale=0.0123, w_scale=None, out_scale=None, b_zp=True):
        g = qlinear_cases.gen(seed)
        rng = np.random.default_rng(seed)
        self.M, self.K, self.N, self.x_mode, self.out_mode = M, K, N, x_mode, out_mode
        self.x_dt, self.w_dt, self.out_dt = DT[x_dt], DT[w_dt], DT[out_dt]
        self.x_zp = zero_point(g, x_zp, self.x_dt) if x_mode == "static" else None
        self.x_scale = torch.tensor(x_scale, dtype=torch.float32, device="cuda") if x_mode == "static" else None
        if x is None:
            if x_mode == "static":
                lo, hi = RANGE[self.x_dt]
                zx = 0 if self.x_zp is None else int(self.x_zp)
                x = ((rng.integers(lo, hi + 1, (M, K)) - zx + rng.uniform(-0.49, 0.49, (M, K))) * x_scale).astype(F)
            else:
                x = rng.standard_normal((M, K)).astype(F)
        self.x_np, self.x = np.asarray(x, F), torch.from_numpy(np.asarray(x, F)).cuda()
        self.w = qlinear_cases.draw(g, (K, N), self.w_dt) if w is None else w
        cols = N if per_column and N > 1 else 1
        self.w_zp = zero_point(g, w_zp, self.w_dt, cols)
        ws = rng.uniform(0.008, 0.012, cols).astype(F) if w_scale is None else np.full(cols, w_scale, F)
        self.w_scale = torch.from_numpy(ws).cuda()
        self.bias = None
        if gemm:
            B = torch.randint(-(1 << 20), 1 << 20, (N,), device="cuda", generator=g, dtype=torch.int32)
            B[0], B[N - 1] = (1 << 25) + 1, -(1 << 25) - 3                      # beyond 2^24: fp32(B[n]) rounds
            self.bias = (B, torch.tensor(3.1e-5, dtype=torch.float32, device="cuda"), torch.tensor(-77, dtype=torch.int32, device="cuda") if b_zp else None)
        self.out_zp = zero_point(g, out_zp, self.out_dt) if out_mode == "static" else None
        self.out_scale = None
        if out_mode == "static":
            if out_scale is None:                                               # about +-100 levels, not a power of two
                v = restate(*self._restate_args(None, None))[2]
                out_scale = F(max(float(np.abs(v[np.isfinite(v)]).max(initial=0.0)), 1e-3) / 100.0 * 1.0137)
            self.out_scale = torch.tensor(float(out_scale), dtype=torch.float32, device="cuda")
        self.want, self.S, self.v = restate(*self._restate_args(out_mode, self.out_scale))

    def _restate_args(self, out_mode, out_scale):
        cpu = lambda t: None if t is None else t.cpu().numpy()      # noqa: E731
        bias = None if self.bias is None else (cpu(self.bias[0]), float(self.bias[1]), cpu(self.bias[2]))
        return (self.x_np, self.x_mode, self.x_dt, None if self.x_scale is None else float(self.x_scale), cpu(self.x_zp), cpu(self.w), cpu(self.w_scale),
                cpu(self.w_zp), bias, out_mode, self.out_dt, None if out_scale is None else float(out_scale), cpu(self.out_zp))

    def kwargs(self):
        return dict(x_mode=self.x_mode, x_scale=self.x_scale, x_zero_point=self.x_zp, out_mode=self.out_mode, out_scale=self.out_scale,
                    out_zero_point=self.out_zp, bias=self.bias)

    def call(self, ops, x=None):
        return ops.qdq_function(self.x if x is None else x, self.w, self.w_scale, self.w_zp, **self.kwargs())


def same_bytes(got, want):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.shape == want.shape and got.dtype == want.dtype == F and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def where_wrong(got, want):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    return f"{len(bad)} of {got.size} differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}" if len(bad) else "equal"


def raw(lib, c, *, x=None, lda=None, w=None, ldw=None, y=None, ldy=None, atype=F32, wtype=None, granularity=None, group_size=0, x_mode=None,
        out_mode=None, workspace_bytes=None):
    """`oq_qdq_function` on QCase `c`; `x`, `w`, `y` may be views with gaps.  (status, y)."""
    x = c.x if x is None else x
    w = c.w if w is None else w
    lda = (x.stride(0) if x.shape[0] > 1 else x.shape[1]) if lda is None else lda
    ldw = (w.stride(0) if w.shape[0] > 1 else w.shape[1]) if ldw is None else ldw
    if y is None:
        y = torch.empty((c.M, c.N), dtype=torch.float32, device="cuda")
    ldy = (y.stride(0) if y.shape[0] > 1 else y.shape[1]) if ldy is None else ldy
    xm, om = MODE[c.x_mode] if x_mode is None else x_mode, MODE[c.out_mode] if out_mode is None else out_mode
    need = lib.oq_qdq_function_workspace_bytes(c.M, c.K, c.N, xm, om)
    assert need == workspace(c.M, c.K, c.N, xm, om)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    per_column = c.w_scale.numel() > 1
    w_zp = c.w_zp if c.w_zp is None or c.w_zp.numel() == c.w_scale.numel() else c.w_zp.reshape(1).expand(c.N).contiguous()
    B, b_scale, b_zp = c.bias if c.bias is not None else (None, None, None)
    st = lib.oq_qdq_function(x.data_ptr(), atype, c.M, c.K, lda, xm, CODE[c.x_dt], ptr(c.x_scale), ptr(c.x_zp), w.data_ptr(),
                             WTYPE[c.w_dt] if wtype is None else wtype, c.N, ldw, (CHANNEL if per_column else TENSOR) if granularity is None else granularity,
                             group_size, ptr(c.w_scale), ptr(w_zp), ptr(B), ptr(b_scale), ptr(b_zp), om, CODE[c.out_dt], ptr(c.out_scale), ptr(c.out_zp),
                             y.data_ptr(), ldy, ws.data_ptr(), need if workspace_bytes is None else workspace_bytes,
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()                                 # `ws` is freed on return
    return st, y
