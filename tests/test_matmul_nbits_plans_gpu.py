"""`oq_matmul_nbits` over the launch plans and tile slots the exact tests of test_matmul_nbits_gpu.py do not enter: k-loops of
several steps on the split-K path and in one block, splits that begin inside a group, every slot of the 128-row tile, several row
tiles with a tail, group sizes that are no power of two, and the `lo` piece of an fp32 A.

Every numeric assertion is bit equality with the float64 reference rounded once, on data whose every partial sum is exact in fp32
in any order.  Every case first asserts the plan it claims (nbits_cases.plan, the formula of include/oq_hip_nbits.h) and that the
library's workspace query is the header's P + S for that number of splits: a change to `make_plan` fails here by name and does
not leave the cases passing in some other plan."""
import numpy as np
import pytest
import torch

from nbits_cases import ATYPE, DTYPES, Case, Plan, describe, gen, workspace

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from onnx_quantize_amd.hip import ops
    return ops


@pytest.fixture(scope="module")
def lib():
    from onnx_quantize_amd.hip import _lib
    return _lib.load()


def assert_plan(lib, c, expected):
    pl = c.plan()
    assert pl == expected, (c.M, c.K, c.N, pl, expected)
    assert lib.oq_matmul_nbits_workspace_bytes(c.M, c.K, c.N, c.group, ATYPE[c.dtype]) == workspace(c.M, c.K, c.N, c.dtype, expected.splits)
    return pl


# ------------------------------------------------------------------------------------ 1. the plan sweep
# (M, K, N), group sizes, Plan(bm, tiles_m, tiles_n, steps, steps_per_split, splits, steps of the last split), what the row adds
SWEEP = [
    ((128, 256, 128), (32, 64, 128, 256), Plan(128, 1, 1, 4, 1, 4, 1), "every slot of the 128-row tile live"),
    ((200, 576, 130), (64, 192), Plan(128, 2, 2, 9, 2, 5, 1), "two-step splits, a short last split, a split boundary inside a group of 192"),
    ((257, 320, 129), (32, 160), Plan(128, 3, 2, 5, 1, 5, 1), "three row tiles with a one-row tail, g = 160"),
    ((32, 576, 260), (96, 288), Plan(32, 1, 3, 9, 2, 5, 1), "a full 32-row tile, g = 96"),
    ((5, 1088, 130), (64, 128), Plan(32, 1, 2, 17, 3, 6, 2), "three-step splits, a tail group of 64 at g = 128"),
    ((130, 1344, 40), (64, 448), Plan(128, 2, 1, 21, 3, 7, 3), "the longest K that is still exact at 8 bits"),
    ((96, 1050, 128), (32, 96), Plan(128, 1, 1, 17, 3, 6, 2), "K % 8 = 2 (narrow A loads), tail groups of 26 and 90"),
    ((8, 200, 16384), (32, 128), Plan(32, 1, 128, 4, 4, 1, 4), "four steps in one block without slabs, 32-row kernel"),
    ((1000, 200, 2000), (32, 128), Plan(128, 8, 16, 4, 4, 1, 4), "the same for the 128-row kernel, M and N tails across the tile index"),
]


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_integers_over_the_plan_sweep(ops, lib, dt, bits):
    """Integers |a| <= 4, scales in {1/8, 1/2, 1}, integer bias, padded positions all-ones, |q - zp| up to 255 and K <= 1344: every
    partial sum is a multiple of 1/8 below 2^24 / 8 (1344 * 4 * 255 * 8 < 2^24), exact in fp32 in any order, so Y IS Y64 rounded
    once.  Zero points alternate between present and absent from case to case, the scales between fp32 and A's type (1/8, 1/2, 1
    are exact in both) from row to row, starting the other way round at 8 bits.  All cases run; the failures are reported
    together, each with its place in the tile."""
    dtype = DTYPES[dt]
    g = gen(300 + bits)
    failures, count = [], 2 if bits == 8 else 0
    for shape, groups, expected, adds in SWEEP:
        for group in groups:
            zero_points, native_scales = count % 2 == 0, (count // 2) % 2 == 1
            count += 1
            c = Case(g, *shape, group, bits, dtype, integer=True, zero_points=zero_points, scale_dtype=dtype if native_scales else torch.float32)
            pl = assert_plan(lib, c, expected)
            assert c.magnitude().max().item() * 8 < 2 ** 24
            wrong = c.run(ops) != c.rounded(c.y64())
            if wrong.any():
                failures.append(f"{shape} g={group} zp={zero_points} scales={'A' if native_scales else 'fp32'} ({adds}): {describe(wrong, pl)}")
    assert not failures, "\n" + "\n".join(failures)


# ------------------------------------------------------------------------------------ 2. the two pieces of an fp32 A
def two_piece_values(g, M, K, dtype):
    """m 2^-10 with 2048 <= |m| <= 4096: under the row's power-of-two scale (largest in [2^14, 2^15)) x s is an integer below
    2^15, hi its fp16 rounding, the residue an integer of at most 8 -- lo is exact, and nonzero wherever x s is no fp16 value."""
    m = torch.randint(2048, 4097, (M, K), device="cuda", generator=g)
    sign = torch.randint(0, 2, (M, K), device="cuda", generator=g) * 2 - 1
    return (m * sign).to(dtype) * 2.0 ** -10


def restated_split(x):
    """csrc/matmul_nbits.hip, nbits_split_rows_kernel, restated in NumPy: (x s, hi, lo) as float32 arrays."""
    x = x.cpu().numpy()
    exponent = np.frexp(np.abs(x).max(axis=1, keepdims=True))[1]                  # largest in [2^(e - 1), 2^e)
    xs = np.ldexp(x, 15 - exponent).astype(np.float32)
    hi = xs.astype(np.float16).astype(np.float32)
    hi[np.abs(hi) < 2.0 ** -14] = 0.0                                             # no fp16 subnormal as hi
    lo = ((xs - hi) * np.float32(2048.0)).astype(np.float16).astype(np.float32)
    return xs, hi, lo


TWO_PIECE_SHAPES = [((128, 128, 128), 32, Plan(128, 1, 1, 2, 1, 2, 1)), ((128, 128, 128), 128, Plan(128, 1, 1, 2, 1, 2, 1)),
                    ((16, 128, 40), 64, Plan(32, 1, 1, 2, 1, 2, 1))]


@pytest.mark.parametrize("bits", [4, 8])
def test_fp32_rows_whose_lo_piece_is_exact_and_nonzero(ops, lib, bits):
    """All terms are multiples of 2^-11 (A: 2^-10, scales 1/2 and 1, an integer bias), and S 2^11 < 2^24 is asserted from the
    float64 reference: every partial sum of hi and lo products is exact in fp32, so Y IS Y64, bit for bit.  4 bits over the whole
    range of q; 8 bits within 15 of the zero point, which keeps S below the limit.  A kernel that loses, misplaces or rescales a
    lo piece is off by at least 2^-11 somewhere."""
    g = gen(500 + bits)
    failures = []
    for shape, group, expected in TWO_PIECE_SHAPES:
        for zero_points in (True, False):
            c = Case(g, *shape, group, bits, torch.float32, integer=True, zero_points=zero_points, scale_values=(0.5, 1.0),
                     q_span=None if bits == 4 else 15, a_values=two_piece_values)
            pl = assert_plan(lib, c, expected)
            xs, hi, lo = restated_split(c.x)
            assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64) * 2.0 ** -11, xs.astype(np.float64))
            assert np.array_equal(xs, np.round(xs)) and np.abs(xs).max() < 2 ** 15 and np.abs(lo).max() <= 8 * 2048
            share = float((lo != 0).mean())
            assert share >= 0.25, share
            assert c.magnitude().max().item() * 2 ** 11 < 2 ** 24
            d = (c.q.reshape(c.N, -1, group) - c.zp[:, :, None]).reshape(c.N, -1)[:, :c.K]
            assert d.abs().max().item() == (15 if zero_points or bits == 8 else 8)
            y64 = c.y64()
            assert torch.equal(y64.float().double(), y64)                          # the reference itself is an fp32 value
            wrong = c.run(ops) != y64.float()
            if wrong.any():
                failures.append(f"{shape} g={group} zp={zero_points}, lo != 0 in {share:.2f}: {describe(wrong, pl)}")
    assert not failures, "\n" + "\n".join(failures)


@pytest.mark.parametrize("bits", [4, 8])
def test_an_fp32_element_whose_hi_would_be_subnormal_arrives_through_lo(ops, lib, bits):
    """Rows hold 4.0 at k0 and j 2^-27 elsewhere, j = 1 .. 8 cycling, and q[:, k0] = zp: the 4.0 fixes the row scale (2^12) and
    contributes nothing.  j 2^-15 is an fp16 subnormal for j = 1 -- hi is zero and the element arrives through lo --, a normal
    hi for j >= 2.  Sums of at most 128 terms j d 2^-27 (and 1/8 of them) and an integer bias: Y64 rounded once."""
    (M, K, N), group, expected = (16, 128, 40), 64, Plan(32, 1, 1, 2, 1, 2, 1)
    k0 = 70

    def values(g, M, K, dtype):
        j = ((torch.arange(M, device="cuda")[:, None] + torch.arange(K, device="cuda")[None, :]) % 8 + 1).to(dtype)
        x = j * 2.0 ** -27
        x[:, k0] = 4.0
        return x

    def zero_at_k0(q, zp):
        q[:, k0] = zp[:, k0 // group]

    for zero_points in (True, False):
        c = Case(gen(600 + bits), M, K, N, group, bits, torch.float32, integer=True, zero_points=zero_points, a_values=values, q_edit=zero_at_k0)
        pl = assert_plan(lib, c, expected)
        assert (c.w64[:, k0] == 0).all()
        xs, hi, lo = restated_split(c.x)
        tiny = (c.x == 2.0 ** -27).cpu().numpy()
        assert tiny.any() and (hi[tiny] == 0).all() and (lo[tiny] == 2.0 ** -4).all()                  # j = 1: through lo
        assert (hi[~tiny] == xs[~tiny]).all() and (lo[~tiny] == 0).all()                                # j >= 2 and the 4.0: a normal hi
        wrong = c.run(ops) != c.rounded(c.y64())
        assert not wrong.any(), describe(wrong, pl)
