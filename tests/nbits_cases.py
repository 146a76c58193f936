"""What the MatMulNBits tests share (test_matmul_nbits_gpu.py, test_matmul_nbits_plans_gpu.py, test_nbits_cases.py):

`Case`       one node and one input on the device, with its float64 reference Y64;
`plan`       the launch plan `make_plan` (csrc/matmul_nbits.hip) derives from (M, K, N), restated from include/oq_hip_nbits.h;
`workspace`  the header's P + S for that plan;
`locate`     wrong output positions -> counts per slot of the kernel's tile, so that a failure reads "row tile 1, wm 1, mt 2, row 12"
             and not like a tensor diff.
"""
import collections

import torch

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
ATYPE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}                 # oq_nbits_type
UNIT = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def pack_blob(q, bits):
    """q [N, blocks, g] uint8 values -> the MatMulNBits blob [N, blocks, g * bits / 8] (4 bits: the even k in the low nibble)."""
    return q.contiguous() if bits == 8 else (q[..., 0::2] | (q[..., 1::2] << 4)).contiguous()


def pack_zero_points(zp, bits):
    """zp [N, blocks] uint8 -> uint8 [N, blocks] (8 bits) or two per byte, low nibble first, the pad nibble of an odd count 0xF."""
    if bits == 8:
        return zp.contiguous()
    if zp.shape[1] % 2:
        zp = torch.cat([zp, torch.full_like(zp[:, :1], 0xF)], dim=1)
    return (zp[:, 0::2] | (zp[:, 1::2] << 4)).contiguous()


# ------------------------------------------------------------------------------------ the launch plan
def ceil_div(a, b):
    return -(-a // b)


def r256(n):
    return (n + 255) // 256 * 256


class Plan(collections.namedtuple("Plan", "bm tiles_m tiles_n steps steps_per_split splits last")):
    """bm: rows of a block tile (32 for M <= 32, else 128); tiles_m x tiles_n block tiles of bm x 128; steps: 64-deep k-steps;
    `splits` workgroups along K (blockIdx.y) of `steps_per_split` steps each, the last one of `last`."""
    __slots__ = ()

    @property
    def tiles(self):
        return self.tiles_m * self.tiles_n


def plan(M, K, N):
    """include/oq_hip_nbits.h, `workspace`: BM, tiles, steps, want, splits."""
    bm = 32 if M <= 32 else 128
    tiles_m, tiles_n = ceil_div(M, bm), ceil_div(N, 128)
    tiles = tiles_m * tiles_n
    steps = ceil_div(K, 64)
    want = 1 if tiles >= 128 else min(8, steps, 256 // tiles)
    steps_per_split = ceil_div(steps, want)
    splits = ceil_div(steps, steps_per_split)
    return Plan(bm, tiles_m, tiles_n, steps, steps_per_split, splits, steps - (splits - 1) * steps_per_split)


def workspace(M, K, N, dtype, splits):
    """The header's P + S: the two fp16 pieces and a scale exponent per row of an fp32 A, and the slabs of `splits` > 1."""
    pieces = 2 * r256(M * 8 * ceil_div(K, 8) * 2) + r256(M * 4) if dtype == torch.float32 else 0
    return pieces + (r256(splits * M * N * 4) if splits > 1 else 0)


# ------------------------------------------------------------------------------------ where a wrong output sits in the tile
Slot = collections.namedtuple("Slot", "row_tile col_tile wm wn mt nt row")


def _slots(mismatch_mask, pl):
    """The distinct slots among the wrong positions, [S, 7] in the order of `Slot`, and how often each occurs, [S]; tensor
    arithmetic throughout, so that a call which got millions of outputs wrong is still reported at once."""
    wrong = torch.nonzero(torch.as_tensor(mismatch_mask))
    m, n = wrong[:, 0], wrong[:, 1]
    r, c, half = m % pl.bm, n % 128, pl.bm // 2                # half: the rows of a wave, 16 * MT
    fields = [m // pl.bm, n // 128, r // half, c // 64, (r % half) // 16, (c % 64) // 16, r % 16]
    sizes = [pl.tiles_m, pl.tiles_n, 2, 2, half // 16, 4, 16]
    key = torch.zeros_like(m)
    for f, size in zip(fields, sizes):
        key = key * size + f
    key, counts = torch.unique(key, return_counts=True)
    columns = []
    for size in reversed(sizes):
        columns.append(key % size)
        key = key // size
    return torch.stack(columns[::-1], dim=1).cpu(), counts.cpu()


def locate(mismatch_mask, pl):
    """mismatch_mask [M, N] bool -> {Slot: count}.  The kernel's map (csrc/matmul_nbits.hip): a block owns bm x 128 outputs;
    wave (wm, wn) of its 2 x 2 owns rows wm * bm / 2 ... and columns wn * 64 ...; there MFMA tile (mt, nt) is 16 x 16, and `row`
    is the row 0 .. 15 inside it (accumulator register row & 3 of lanes 16 (row >> 2) ... + 15)."""
    slots, counts = _slots(mismatch_mask, pl)
    return {Slot(*s): k for s, k in zip(slots.tolist(), counts.tolist())}


def describe(mismatch_mask, pl, most=8):
    """`locate` as one line: the number of wrong outputs, per coordinate the values that occur among them, the slots hit most."""
    slots, counts = _slots(mismatch_mask, pl)
    if not len(counts):
        return "no mismatch"
    parts = [f"{name} {compact(torch.unique(slots[:, i]).tolist())}" for i, name in enumerate(Slot._fields)]
    order = torch.argsort(counts, descending=True, stable=True)[:most]
    worst = ", ".join(f"{tuple(slots[i].tolist())} x{int(counts[i])}" for i in order)
    return f"{int(counts.sum())} wrong in {len(counts)} slots: " + ", ".join(parts) + "; most hit: " + worst


def compact(values):
    """[0, 1, 2, 3, 7] -> '[0-3, 7]'."""
    runs, start = [], 0
    for i in range(1, len(values) + 1):
        if i == len(values) or values[i] != values[i - 1] + 1:
            runs.append(str(values[start]) if i - 1 == start else f"{values[start]}-{values[i - 1]}")
            start = i
    return "[" + ", ".join(runs) + "]"


# ------------------------------------------------------------------------------------ a node and an input
class Case:
    """One node and one input: the device tensors `ops.matmul_nbits` takes, and Y64.

    q_span        q is drawn within +- q_span of its zero point (None: the whole range of `bits`).
    scale_values  the values integer data draws its scales from.
    a_values      a callable (generator, M, K, dtype) -> A [M, K], in place of the drawn A.
    q_edit        a callable (q [N, blocks * g] int32, zp [N, blocks] int32), editing q in place before it is packed.

    Extremes are forced in every case: per 128-column tile one (q, zp) pair is (0, top) and one is (top, 0), top = 2^bits - 1, so
    that d = q - zp = -+top occurs (with q_span: -+q_span; without zero points: the ends of q's range around 2^(bits - 1)).  The
    pairs sit at k = 0 of the tile's first two columns -- or, where the tile has one column, at the first k of its first two
    groups; a tile of one column and one group gets the first pair only."""

    def __init__(self, g, M, K, N, group, bits, dtype, *, zero_points=True, bias=True, integer=False, scale_dtype=torch.float32,
                 q_span=None, scale_values=(0.125, 0.5, 1.0), a_values=None, q_edit=None):
        self.M, self.K, self.N, self.group, self.bits, self.dtype = M, K, N, group, bits, dtype
        blocks = (K + group - 1) // group
        top = (1 << bits) - 1
        if zero_points:
            zp = torch.randint(0, top + 1, (N, blocks), device="cuda", generator=g, dtype=torch.int32)
        else:
            zp = None
        zp_used = zp if zp is not None else torch.full((N, blocks), 1 << (bits - 1), device="cuda", dtype=torch.int32)
        span = top if q_span is None else q_span
        first = torch.arange(0, N, 128, device="cuda")             # (column, group 0) of every tile: zp = top, q as far below as allowed
        alone = first + 1 >= N                                     # the tile has this one column
        keep = ~alone if blocks == 1 else torch.ones_like(alone)
        second_n, second_kb = torch.where(alone, first, first + 1)[keep], alone.long()[keep]
        if zp is not None:                                         # before q is drawn around the zero points
            zp[first, 0] = top
            zp[second_n, second_kb] = 0
        if q_span is None:
            q = torch.randint(0, top + 1, (N, blocks * group), device="cuda", generator=g, dtype=torch.int32)
        else:
            d = torch.randint(-q_span, q_span + 1, (N, blocks, group), device="cuda", generator=g, dtype=torch.int32)
            q = (zp_used[:, :, None] + d).clamp_(0, top).reshape(N, blocks * group)
        q[first, 0] = (zp_used[first, 0] - span).clamp_(min=0)
        q[second_n, second_kb * group] = (zp_used[second_n, second_kb] + span).clamp_(max=top)
        if q_edit is not None:
            q_edit(q, zp_used)
        q[:, K:] = top                                             # every padded position: all bits set (0xFF bytes in the blob)
        if integer:
            a = torch.randint(-4, 5, (M, K), device="cuda", generator=g).to(dtype)
            values = torch.tensor(scale_values, device="cuda")
            scales = values[torch.randint(0, len(scale_values), (N, blocks), device="cuda", generator=g)]
            b = torch.randint(-8, 9, (N,), device="cuda", generator=g).to(dtype) if bias else None
        else:
            a = torch.randn((M, K), device="cuda", generator=g).to(dtype)
            scales = (torch.rand((N, blocks), device="cuda", generator=g) * 0.02 + 0.001)
            b = torch.randn((N,), device="cuda", generator=g).to(dtype) if bias else None
        if a_values is not None:
            a = a_values(g, M, K, dtype)
            assert a.shape == (M, K) and a.dtype == dtype and a.device == q.device
        self.x, self.bias = a, b
        self.scales = scales.to(scale_dtype)
        self.q, self.zp = q, zp_used                               # as drawn: what a test restates the operands from
        self.blob = pack_blob(q.to(torch.uint8).reshape(N, blocks, group), bits)
        self.zero_points = None if zp is None else pack_zero_points(zp.to(torch.uint8), bits)
        zp64 = zp_used.to(torch.float64)
        w = (q.reshape(N, blocks, group).to(torch.float64) - zp64[:, :, None]) * self.scales.to(torch.float64)[:, :, None]
        self.w64 = w.reshape(N, blocks * group)[:, :K].contiguous()

    def y64(self, x=None):
        y = (self.x if x is None else x).to(torch.float64) @ self.w64.t()
        return y if self.bias is None else y + self.bias.to(torch.float64)

    def magnitude(self, x=None):
        """S = |A| . |w|^T + |bias| in float64: what every error term of the kernel is a multiple of."""
        s = (self.x if x is None else x).to(torch.float64).abs() @ self.w64.abs().t()
        return s if self.bias is None else s + self.bias.to(torch.float64).abs()

    def bound(self, x=None):
        """|Y - Y64| allowed, elementwise (the module docstring of test_matmul_nbits_gpu.py)."""
        x64 = (self.x if x is None else x).to(torch.float64)
        s = self.magnitude(x)
        blocks = (self.K + self.group - 1) // self.group
        term = (self.K + 2 * blocks + 4) * 2.0 ** -23 * s
        if self.dtype == torch.float32:           # the two-piece operand: 22 bits, doubled; elements below 2^-17 of their row's largest
            term = term + 2.0 ** -21 * s + self.K * 2.0 ** -38 * x64.abs().amax(dim=1, keepdim=True) * self.w64.abs().max()
        return term + UNIT[self.dtype] * (self.y64(x).abs() + term)

    def run(self, ops, x=None):
        return ops.matmul_nbits(self.x if x is None else x, self.blob, self.scales, self.zero_points, K=self.K, N=self.N, bits=self.bits,
                                block_size=self.group, bias=self.bias)

    def parent(self, x=None):
        """The expansion route a holder of a quantized file had before the kernel: `GraphRunner._op_MatMulNBits` itself."""
        from onnx_quantize_amd.graph_runner import GraphRunner
        runner = GraphRunner.evaluator(21)
        attrs = {"K": self.K, "N": self.N, "bits": self.bits, "block_size": self.group}
        return GraphRunner._op_MatMulNBits(runner, None, [self.x if x is None else x, self.blob, self.scales, self.zero_points, None, self.bias],
                                           attrs, None)

    def rounded(self, y64):
        return y64.float().to(self.dtype)

    def plan(self):
        return plan(self.M, self.K, self.N)

    def workspace(self):
        return workspace(self.M, self.K, self.N, self.dtype, self.plan().splits)
