"""What the tests of the QDQ functions' fused product share (test_qdq_matmul_gpu.py, test_qdq_runner_gpu.py):

`Case`      one weight as a QDQ file stores it -- W [K, N] one byte per value, its scales and zero points per tensor, per column
            or per group of K -- and one input, on the device, with the float64 reference Y64.  It IS an `nbits_cases.Case` in
            everything that judges a result (`y64`, `magnitude`, `bound`, `rounded`, `plan`, `workspace`): the arithmetic of
            `oq_qdq_matmul` is that of `oq_matmul_nbits`, so the bound is that derivation with blocks = K / g, or 1 per tensor /
            per column, and not a new number.
`describe`  `nbits_cases.describe`: the kernel's tile (rows x 128 columns, 2 x 2 waves, 16 x 16 MFMA tiles) is the same.
"""
import torch

import nbits_cases
from nbits_cases import ATYPE, DTYPES, describe, gen      # noqa: F401 -- re-exported for the tests

WTYPE = {torch.int8: 2, torch.uint8: 3}                      # oq_qtype: OQ_INT8, OQ_UINT8
GRANULARITY = {"tensor": 0, "column": 1, "group": 2}         # oq_strategy


class Case(nbits_cases.Case):
    """granularity: "tensor", "column", or the group size (an int).

    Extremes are forced in every case.  With zero points per column or per group: per 128-column tile one (q, zp) pair is
    (lo, hi) and one is (hi, lo), lo / hi the ends of W's type, so that d = q - zp = -+255 occurs; they sit at k = 0 of the tile's
    first two columns -- or, where the tile has one column, at the first k of its first two groups; a tile of one column and one
    group gets the first pair only.  Per tensor, and without zero points, the ends of W's type itself are forced at those places
    (the one zero point is drawn)."""

    def __init__(self, g, M, K, N, granularity, dtype, wdtype=torch.uint8, *, zero_points=True, bias=True, integer=False,
                 scale_dtype=torch.float32, scale_values=(0.125, 0.5, 1.0)):
        grouped = not isinstance(granularity, str)
        group = int(granularity) if grouped else K
        assert K % group == 0
        self.M, self.K, self.N, self.group, self.dtype, self.wdtype = M, K, N, group, dtype, wdtype
        self.granularity = "group" if grouped else granularity
        self.group_size = group if grouped else 0
        blocks = K // group
        lo, hi = (0, 255) if wdtype == torch.uint8 else (-128, 127)
        shape = (1, 1) if granularity == "tensor" else (N, blocks)
        zp = torch.randint(lo, hi + 1, shape, device="cuda", generator=g, dtype=torch.int32) if zero_points else None
        q = torch.randint(lo, hi + 1, (N, K), device="cuda", generator=g, dtype=torch.int32)       # [n, k] while it is drawn
        first = torch.arange(0, N, 128, device="cuda")
        alone = first + 1 >= N
        keep = ~alone if blocks == 1 else torch.ones_like(alone)
        second_n, second_kb = torch.where(alone, first, first + 1)[keep], alone.long()[keep]
        if zp is not None and granularity != "tensor":
            zp[first, 0] = hi
            zp[second_n, second_kb] = lo
        q[first, 0] = lo
        q[second_n, second_kb * group] = hi
        if integer:
            a = torch.randint(-4, 5, (M, K), device="cuda", generator=g).to(dtype)
            values = torch.tensor(scale_values, device="cuda")
            scales = values[torch.randint(0, len(scale_values), shape, device="cuda", generator=g)]
            b = torch.randint(-8, 9, (N,), device="cuda", generator=g).to(dtype) if bias else None
        else:
            a = torch.randn((M, K), device="cuda", generator=g).to(dtype)
            scales = torch.rand(shape, device="cuda", generator=g) * 0.02 + 0.001
            b = torch.randn((N,), device="cuda", generator=g).to(dtype) if bias else None
        self.x, self.bias = a, b
        self.scales = scales.to(scale_dtype).reshape(-1)                 # flat: 1 | N | N * K / g, entry n * (K / g) + k / g
        self.w = q.t().contiguous().to(wdtype)                           # [K, N], as the file stores it
        self.zero_points = None if zp is None else zp.to(wdtype).reshape(-1)
        zp64 = torch.zeros(shape, device="cuda", dtype=torch.float64) if zp is None else zp.to(torch.float64)
        s64 = self.scales.to(torch.float64).reshape(shape)
        w = (q.reshape(N, blocks, group).to(torch.float64) - zp64.expand(N, blocks)[:, :, None]) * s64.expand(N, blocks)[:, :, None]
        self.w64 = w.reshape(N, K).contiguous()                          # [N, K], the orientation nbits_cases.Case judges with

    def run(self, ops, x=None, w=None):
        return ops.qdq_matmul(self.x if x is None else x, self.w if w is None else w, self.scales, self.zero_points,
                              group_size=self.group_size, bias=self.bias)

    def parent(self, x=None):
        """The expansion route: what the function body does today -- dequantize the whole weight in fp32, then matmul in A's type."""
        x = self.x if x is None else x
        blocks = self.K // self.group
        shape = (1, 1) if self.granularity == "tensor" else (self.N, blocks)
        zp = 0.0 if self.zero_points is None else self.zero_points.float().reshape(shape).expand(self.N, blocks)[:, :, None]
        s = self.scales.float().reshape(shape).expand(self.N, blocks)[:, :, None]
        w = ((self.w.t().float().reshape(self.N, blocks, self.group) - zp) * s).reshape(self.N, self.K).t()
        out = x @ w.to(x.dtype)
        return out if self.bias is None else out + self.bias

    def raw(self, lib, y, ldy, *, x=None, lda=None, w=None, ldw=None, workspace=None, **over):
        """`oq_qdq_matmul` itself on this case, with the overrides a refusal test needs; returns the status."""
        x = self.x if x is None else x
        w = self.w if w is None else w
        raw = lib.load()
        atype = over.pop("atype", ATYPE[self.dtype])
        need = raw.oq_qdq_matmul_workspace_bytes(self.M, self.K, self.N, ATYPE[self.dtype])
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda") if workspace is None else workspace
        self._keep = ws
        a = dict(M=self.M, K=self.K, lda=self.K if lda is None else lda, wtype=WTYPE[self.wdtype], N=self.N, ldw=self.N if ldw is None else ldw,
                 granularity=GRANULARITY[self.granularity], group_size=self.group_size, scales_type=ATYPE[self.scales.dtype],
                 workspace_bytes=need if workspace is None else workspace.numel())
        assert set(over) <= set(a), over
        a.update(over)
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        return raw.oq_qdq_matmul(x.data_ptr(), atype, a["M"], a["K"], a["lda"], w.data_ptr(), a["wtype"], a["N"], a["ldw"], a["granularity"],
                                 a["group_size"], self.scales.data_ptr(), a["scales_type"], ptr(self.zero_points), ptr(self.bias), y.data_ptr(),
                                 ldy, ws.data_ptr(), a["workspace_bytes"], torch.cuda.current_stream().cuda_stream)
