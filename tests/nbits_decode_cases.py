"""What the tests of the decode route of MatMulNBits share (test_matmul_nbits_decode_*.py):

`decode_plan`       the launch plan of csrc/decode_plan.hpp, restated from include/oq_hip_nbits_decode.h;
`decode_workspace`  the header's S for that plan;
`DecodeCase`        a `Case` of nbits_cases.py whose zero points may also be floating point [N, blocks] (HQQ), with the bound of
                    DESIGN.md 4.26 and the exactness precondition of integer data;
`raw_decode`        `oq_matmul_nbits_decode` itself, for what `ops.matmul_nbits_decode` never passes (ldy > N, hostile arguments).
"""
import collections
import ctypes as C

import torch

from nbits_cases import ATYPE, UNIT, Case, ceil_div, r256

ZP_PACKED_U8 = 3                                                  # OQ_NBITS_ZP_PACKED_U8
ZP_FORMS = ("none", "packed", "fp32", "native")                   # absent, uint8 as stored, float32, float of A's type
DecodePlan = collections.namedtuple("DecodePlan", "tier splits rows_per_block row_blocks grid last")


def decode_plan(M, K, N, dtype=None):
    """include/oq_hip_nbits_decode.h, `Plan`; `last`: the k of the last slice."""
    tier = 1 if M == 1 else 4 if M <= 4 else 8 if M <= 8 else 16
    splits = ceil_div(K, 1024)
    want = max(1, (256 if dtype == torch.float32 and tier >= 8 else 512) // splits)
    rows_per_block = 64 * ceil_div(ceil_div(N, want), 64)
    row_blocks = ceil_div(N, rows_per_block)
    return DecodePlan(tier, splits, rows_per_block, row_blocks, row_blocks * splits, K - (splits - 1) * 1024)


def decode_workspace(M, K, N):
    splits = ceil_div(K, 1024)
    return r256(splits * M * N * 4) if splits > 1 else 0


class DecodeCase(Case):
    """`Case` with ``zp`` one of ZP_FORMS.  Float zero points are drawn anew: with ``integer`` multiples of 0.5 in [0, 2^bits - 1]
    (whatever of them the storing type holds: still multiples of 0.5), otherwise uniform in that range."""

    def __init__(self, g, M, K, N, group, bits, dtype, *, zp="packed", **kw):
        super().__init__(g, M, K, N, group, bits, dtype, zero_points=zp != "none", **kw)
        self.zp_form = zp
        blocks = ceil_div(K, group)
        top = (1 << bits) - 1
        if zp in ("fp32", "native"):
            if kw.get("integer"):
                z = torch.randint(0, 2 * top + 1, (N, blocks), device="cuda", generator=g).to(torch.float64) * 0.5
            else:
                z = torch.rand((N, blocks), device="cuda", generator=g, dtype=torch.float64) * top
            self.zero_points = z.to(torch.float32 if zp == "fp32" else dtype)
            self.zp = self.zero_points.to(torch.float64)              # what the file holds
            w = (self.q.reshape(N, blocks, group).to(torch.float64) - self.zp[:, :, None]) * self.scales.to(torch.float64)[:, :, None]
            self.w64 = w.reshape(N, blocks * group)[:, :K].contiguous()
        self.float_zp = zp in ("fp32", "native")

    # S = |A| |w|^T + |bias|, or with float zero points S* = sum |a| (q + |zp|) |s| + |bias|
    def magnitude(self, x=None):
        if not self.float_zp:
            return super().magnitude(x)
        N, K, group = self.N, self.K, self.group
        blocks = ceil_div(K, group)
        w = (self.q.reshape(N, blocks, group).to(torch.float64) + self.zp.abs()[:, :, None]) * self.scales.to(torch.float64).abs()[:, :, None]
        s = (self.x if x is None else x).to(torch.float64).abs() @ w.reshape(N, blocks * group)[:, :K].t()
        return s if self.bias is None else s + self.bias.to(torch.float64).abs()

    def bound(self, x=None):
        """|Y - Y64| <= c 2^-24 S + ulp_out / 2 (|Y64| + that), c = g + blocks + 8."""
        c = self.group + ceil_div(self.K, self.group) + 8
        term = c * 2.0 ** -24 * self.magnitude(x)
        return term + UNIT[self.dtype] * (self.y64(x).abs() + term)

    def exact_in_fp32(self):
        """Integer data: every partial sum is a multiple of the quantum (2^-3: scales down to 1/8; 2^-4 with half-integer zero points)
        below 2^24 of them, so exact in fp32 in any order."""
        quantum = 2.0 ** -4 if self.float_zp else 2.0 ** -3
        s = self.x.to(torch.float64).abs() @ self.w64.abs().t()
        if self.bias is not None:
            s = s + self.bias.to(torch.float64).abs()
        return s.max().item() / quantum < 2 ** 24

    def run(self, ops, x=None):
        return ops.matmul_nbits_decode(self.x if x is None else x, self.blob, self.scales, self.zero_points, K=self.K, N=self.N,
                                       bits=self.bits, block_size=self.group, bias=self.bias)

    def tile(self, ops, x=None):
        return super().run(ops, x)

    def plan(self):
        return decode_plan(self.M, self.K, self.N, self.dtype)

    def workspace(self):
        return decode_workspace(self.M, self.K, self.N)

    def zp_type(self):
        return ZP_PACKED_U8 if not self.float_zp else ATYPE[self.zero_points.dtype]


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def raw_decode(lib, c, out, ldy, *, x=None, lda=None, M=None, bits=None, group=None, flags=0, workspace=None):
    """One call of the entry point on the current stream; returns (status, message)."""
    x = c.x if x is None else x
    M = x.shape[0] if M is None else M
    need = lib.oq_matmul_nbits_decode_workspace_bytes(min(M, 16), c.K, c.N, c.group, ATYPE[c.dtype])
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda") if workspace is None else workspace
    st = lib.oq_matmul_nbits_decode(_ptr(x), ATYPE[c.dtype], M, c.K, c.K if lda is None else lda, _ptr(c.blob), c.bits if bits is None else bits, c.N,
                                    c.group if group is None else group, _ptr(c.scales), ATYPE[c.scales.dtype], _ptr(c.zero_points), c.zp_type(),
                                    _ptr(c.bias), flags, _ptr(out), ldy, _ptr(ws), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, lib.oq_last_error().decode()
