"""What the tests of the float-zero-point tile route of MatMulNBits share (test_matmul_nbits_fzp_*.py; include/oq_hip_nbits_fzp.h,
DESIGN.md 4.30):

`split`     a zero point as the kernel splits it: zi = clamp(rint(zp), 0, 2^bits - 1), f = zp - zi, in float32;
`FzpCase`   a `DecodeCase` (floating-point zero points [N, blocks], float32 or of A's type) whose `run` is
            `ops.matmul_nbits_float_zp`, which can draw its zero points as an HQQ file holds them or integer-valued, plant values
            outside [0, 2^bits - 1] in chosen cells, and which carries the magnitude S' and the bound of DESIGN.md 4.30;
`raw_fzp`   `oq_matmul_nbits_fzp` itself, for what `ops.matmul_nbits_float_zp` never passes (lda, ldy > N, hostile arguments).
"""
import ctypes as C

import torch

from nbits_cases import ATYPE, UNIT, ceil_div, pack_zero_points, plan, workspace
from nbits_decode_cases import DecodeCase


def split(zero_points, bits):
    """(zi, f) of float zero points, restated in torch float32 exactly as csrc/matmul_nbits_fzp.hip defines them: rint is
    round-half-to-even (`torch.round`), a NaN gives zi = 0 and f = NaN."""
    zp = zero_points.to(torch.float32)
    top = float((1 << bits) - 1)
    r = torch.round(zp)
    zi = torch.where(r > 0, torch.where(r < top, r, torch.full_like(r, top)), torch.zeros_like(r))
    return zi, zp - zi


class FzpCase(DecodeCase):
    """`DecodeCase` with ``zp`` "fp32" or "native".  ``values`` says how the zero points are drawn:
         None     as `DecodeCase` draws them: uniform in [0, top], with ``integer`` multiples of 0.5 there;
         "hqq"    top / 2 plus uniform noise of width 2, where HQQ's zero points sit;
         "whole"  integers in [0, top]: f = 0 everywhere.
    ``plant``: (n, block, value) cells set afterwards -- values outside [0, top] are legal.  With ``integer`` two ties of rint
    are forced: cell (0, 0) holds 2.5 (-> 2) and, where the row has a second cell, its last one holds 3.5 (-> 4)."""

    def __init__(self, g, M, K, N, group, bits, dtype, *, zp="fp32", values=None, plant=(), **kw):
        assert zp in ("fp32", "native")
        super().__init__(g, M, K, N, group, bits, dtype, zp=zp, **kw)
        blocks, top = ceil_div(K, group), (1 << bits) - 1
        z = self.zp.clone()
        if values == "hqq":
            z = top / 2 + (torch.rand((N, blocks), device="cuda", generator=g, dtype=torch.float64) - 0.5) * 2
        elif values == "whole":
            z = torch.randint(0, top + 1, (N, blocks), device="cuda", generator=g).to(torch.float64)
        else:
            assert values is None
        if kw.get("integer") and values is None:
            z[0, 0] = 2.5
            if blocks > 1:
                z[0, blocks - 1] = 3.5
        for n, block, value in plant:
            z[n, block] = value
        self.zero_points = z.to(torch.float32 if zp == "fp32" else dtype)
        self.zp = self.zero_points.to(torch.float64)                  # what the file holds
        w = (self.q.reshape(N, blocks, group).to(torch.float64) - self.zp[:, :, None]) * self.scales.to(torch.float64)[:, :, None]
        self.w64 = w.reshape(N, blocks * group)[:, :K].contiguous()

    def split(self):
        return split(self.zero_points, self.bits)

    def _weight_magnitude(self):
        """(|q - zi| + |f|) |s|, [N, K] float64."""
        N, K, group = self.N, self.K, self.group
        blocks = ceil_div(K, group)
        zi, f = self.split()
        w = ((self.q.reshape(N, blocks, group).to(torch.float64) - zi.to(torch.float64)[:, :, None]).abs() + f.to(torch.float64).abs()[:, :, None])
        return (w * self.scales.to(torch.float64).abs()[:, :, None]).reshape(N, blocks * group)[:, :K]

    def magnitude(self, x=None):
        """S' = sum |a| (|q - zi| + |f|) |s| + |bias| in float64: what every error term of the kernel is a multiple of."""
        s = (self.x if x is None else x).to(torch.float64).abs() @ self._weight_magnitude().t()
        return s if self.bias is None else s + self.bias.to(torch.float64).abs()

    def bound(self, x=None):
        """|Y - Y64| allowed, elementwise: the bound of `Case.bound` on S', with one more rounding per group for
        the correction's fma; an fp32 A adds the two terms of its pieces, on (|q - zi| + |f|) |s| in place of |w|."""
        x64 = (self.x if x is None else x).to(torch.float64)
        s = self.magnitude(x)
        blocks = ceil_div(self.K, self.group)
        term = (self.K + 3 * blocks + 4) * 2.0 ** -23 * s
        if self.dtype == torch.float32:
            term = term + 2.0 ** -21 * s + self.K * 2.0 ** -38 * x64.abs().amax(dim=1, keepdim=True) * self._weight_magnitude().max()
        return term + UNIT[self.dtype] * (self.y64(x).abs() + term)

    def exact_in_fp32(self):
        """Integer data: A integers, zi integers, f and the zero points multiples of 1/2, scales down to 1/8 -- every partial sum is a
        multiple of 2^-4 and at most S', so below 2^24 quanta it is exact in fp32 in any order."""
        return self.magnitude().max().item() / 2.0 ** -4 < 2 ** 24

    def run(self, ops, x=None):
        return ops.matmul_nbits_float_zp(self.x if x is None else x, self.blob, self.scales, self.zero_points, K=self.K, N=self.N,
                                         bits=self.bits, block_size=self.group, bias=self.bias)

    def decode(self, ops, x=None):
        return DecodeCase.run(self, ops, x)

    def packed(self, ops, x=None):
        """`ops.matmul_nbits` on the same blob with the zero points rounded (rint) and packed: the same product only where they are
        whole numbers inside the range."""
        zi, _ = self.split()
        return ops.matmul_nbits(self.x if x is None else x, self.blob, self.scales, pack_zero_points(zi.to(torch.uint8), self.bits), K=self.K,
                                N=self.N, bits=self.bits, block_size=self.group, bias=self.bias)

    def plan(self):
        return plan(self.M, self.K, self.N)

    def workspace(self):
        return workspace(self.M, self.K, self.N, self.dtype, self.plan().splits)


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def raw_fzp(lib, c, out, ldy, *, x=None, lda=None, bits=None, group=None, flags=0, zero_points="own", zp_type=None, workspace=None):
    """One call of the entry point on the current stream; returns (status, message)."""
    x = c.x if x is None else x
    M = x.shape[0]
    need = lib.oq_matmul_nbits_fzp_workspace_bytes(M, c.K, c.N, c.group, ATYPE[c.dtype])
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda") if workspace is None else workspace
    zp = c.zero_points if isinstance(zero_points, str) else zero_points
    st = lib.oq_matmul_nbits_fzp(_ptr(x), ATYPE[c.dtype], M, c.K, x.stride(0) if lda is None else lda, _ptr(c.blob), c.bits if bits is None else bits,
                                 c.N, c.group if group is None else group, _ptr(c.scales), ATYPE[c.scales.dtype], _ptr(zp),
                                 ATYPE[c.zero_points.dtype] if zp_type is None else zp_type, _ptr(c.bias), flags, _ptr(out), ldy, _ptr(ws), ws.numel(),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, lib.oq_last_error().decode()
