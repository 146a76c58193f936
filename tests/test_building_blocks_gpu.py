"""The small kernels the routes stand on, each held bit for bit against NumPy at the edges no other test reaches:
csrc/elementwise.hip (Q1, K1, K2, A3 and the wire-format packers) and `minmax_rows` of csrc/reduce.hip.

Every expectation is the oracle's NumPy restatement or a few lines of NumPy (building_block_cases.py); there is no tolerance and
no allowed share of mismatches anywhere in this file.  Two things are NOT compared bit for bit, because IEEE 754 leaves them
open and x86 and the GPU choose differently: the payload / sign of a NaN (NaN-ness is compared instead), and the integer a NaN
becomes in NumPy.

K1 where NumPy's float -> int32 cast is undefined (section 4).  x / scale below; `zp+`, `0`, `zp-` are a positive, zero and
negative zero point.  NumPy: what `oq_oracle.quantize` gives on the x86-64 CPU that made the goldens (every such quotient becomes
INT32_MIN, then the int32 sum wraps).  Kernel: the rule include/oq_hip.h states, clamp(sat32(rint(x / s)) + zp), which
`test_quantize_where_numpy_is_undefined` asserts.

    x / scale      NumPy zp+   NumPy 0   NumPy zp-   |  kernel zp+   kernel 0   kernel zp-
    NaN            qmin        qmin      qmax        |  clamp(zp)    clamp(0)   clamp(zp)
    +inf           qmin        qmin      qmax        |  qmax         qmax       qmax
    -inf           qmin        qmin      qmax        |  qmin         qmin       qmin
    +2^31          qmin        qmin      qmax        |  qmax         qmax       qmax
    -2^31          qmin        qmin      qmax  (*)   |  qmin         qmin       qmin
    +3e9           qmin        qmin      qmax        |  qmax         qmax       qmax
    -3e9           qmin        qmin      qmax        |  qmin         qmin       qmin
    (*) the cast is defined here (INT32_MIN); NumPy's qmax comes from its wrapped int32 sum alone.

`oq_quantize_bias_f32` (zero point 0): NumPy gives INT32_MIN for all seven and for bias / 0; the kernel saturates -- +inf, +2^31,
+3e9, 1 / 0 -> INT32_MAX; -inf, -2^31, -3e9, -1 / 0 -> INT32_MIN; NaN and 0 / 0 -> 0 (`test_bias_where_numpy_is_undefined`).

Q1 (section 5): `oq_oracle.qparams` itself casts a NaN zero point to an integer (platform-defined) for the asymmetric ranges
(NaN, 1), (-1, NaN), (NaN, NaN), (-inf, 1) and (-inf, +inf); for those only the zero point NARROWED to the container dtype is
compared (0 on both sides), for every other range also the int32 the kernel wrote.
"""
import numpy as np
import pytest

import oq_oracle as O
import building_block_cases as B
from building_block_cases import BYTE_TYPES, MODES, dev, host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import torch
    from onnx_quantize_amd.hip import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def same_bytes(got, expected):
    got, expected = np.ascontiguousarray(got), np.ascontiguousarray(expected)
    return got.dtype == expected.dtype and got.shape == expected.shape and got.tobytes() == expected.tobytes()


# ============================================================================= 1. oq_minmax_rows_f32
def _assert_minmax(ops, view, x):
    mn, mx = ops.minmax_rows(view)
    assert same_bytes(host(mn), x.min(axis=1)) and same_bytes(host(mx), x.max(axis=1))


@pytest.mark.parametrize("r,c", [(1, 1), (3, 7), (4, 256), (5, 260), (9, 1028), (6, 63), (130, 4)])
def test_minmax_rows_shapes(ops, r, c):
    """Both arms (float4: C % 4 == 0; scalar), rows shorter and longer than one pass of the wave (64 / 256 columns), 1, 3 and 5
    rows (a last block of one row) and more than one block."""
    x = (np.random.default_rng(r * 1000 + c).standard_normal((r, c)) * 3).astype(np.float32)
    _assert_minmax(ops, dev(x), x)


@pytest.mark.parametrize("r", [1, 3, 5])
@pytest.mark.parametrize("c,ld,offset", [(256, 260, 0), (256, 257, 0), (256, 256, 1), (256, 260, 1), (63, 70, 0)])
def test_minmax_rows_views(ops, r, c, ld, offset):
    """ldx = C + 4: the float4 arm must not read the gap (it holds +-1e30) into the result.  ldx = C + 1 and a base one element
    off 16 bytes: the scalar arm must be taken although C % 4 == 0."""
    import torch
    x = (np.random.default_rng(ld * 10 + offset).standard_normal((r, c)) * 3).astype(np.float32)
    view, buf = B.strided(x, ld, offset, fill=1e30)
    buf.view(-1)[offset + c::2] = -1e30                                   # both signs somewhere in every gap
    view.copy_(dev(x))
    assert view.data_ptr() % 16 == (4 * offset) % 16 and (r == 1 or view.stride(0) == ld)
    if r == 1:                                                            # a one-row view has no stride to pass: the C ABI takes ldx
        mn, mx = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
        assert B.L.load().oq_minmax_rows_f32(view.data_ptr(), 1, c, ld, mn.data_ptr(), mx.data_ptr(), B.stream()) == 0
        assert same_bytes(host(mn), x.min(axis=1)) and same_bytes(host(mx), x.max(axis=1))
    else:
        _assert_minmax(ops, view, x)


@pytest.mark.parametrize("c", [63, 260])
def test_minmax_rows_nan_negative_zero_and_infinities(ops, c):
    """A NaN makes exactly its row's min and max NaN, as np.min does; a row of -0.0 keeps its sign; +-inf are extrema."""
    x = (np.random.default_rng(c).standard_normal((7, c)) * 3).astype(np.float32)
    x[2, c // 2] = np.nan
    x[4, :] = -0.0
    x[5, 1], x[5, c - 2] = np.inf, -np.inf
    x[6, c - 1] = np.inf
    emn, emx = B.quiet(np.min, x, axis=1), B.quiet(np.max, x, axis=1)
    mn, mx = (host(t) for t in ops.minmax_rows(dev(x)))
    bad = np.arange(7) == 2
    assert np.array_equal(np.isnan(emn), bad) and np.array_equal(np.isnan(mn), bad) and np.array_equal(np.isnan(mx), bad)
    assert same_bytes(mn[~bad], emn[~bad]) and same_bytes(mx[~bad], emx[~bad])
    assert np.signbit(mn[4]) and np.signbit(mx[4]) and mx[5] == np.inf and mn[5] == -np.inf


def test_functional_min_max_reaches_the_row_kernel():
    """`_compute_min_max` for channel / group is the kernel's only caller in the package (utils.py:42-69: zero joins the range)."""
    from onnx_quantize_amd import QuantizationStrategy
    from onnx_quantize_amd.algorithms import functional as F
    rows = (np.random.default_rng(5).standard_normal((13, 96)) + 0.5).astype(np.float32)
    rows[3] = np.abs(rows[3]) + 1                                          # a strictly positive row: its minimum becomes 0
    lo, hi = F._compute_min_max(rows, QuantizationStrategy.CHANNEL, clip_ratio=0.9)
    elo, ehi = O.min_max(rows, "channel", np.float32(0.9))
    assert same_bytes(lo, elo) and same_bytes(hi, ehi)


# ============================================================================= 2. K1 / K2 on paths that never ran
def _draw(seed, qtype, mode, r, c, group):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((r, c)) * 3).astype(np.float32)
    scale, zp = B.draw_params(rng, qtype, B.param_count(mode, r, c, group))
    s_full, z_full = B.expand(mode, r, c, group, scale), B.expand(mode, r, c, group, zp)
    eq = O.quantize(x, s_full, z_full, qtype, False, False)
    return x, scale, zp, eq, O.dequantize(eq, s_full, z_full)


@pytest.mark.parametrize("qtype", ["uint8", "int4"])
@pytest.mark.parametrize("mode,group", [("col", 1), ("group", 41)])
def test_generic_kernels_past_one_grid_trip(ops, qtype, mode, group):
    """1025 x 1031 = 1 056 775 elements > 4096 blocks x 256 threads, C odd (no tile path): the grid-stride loops of
    quantize_kernel / dequantize_kernel take a second trip, and only part of the grid does."""
    r, c = 1025, 1031
    assert r * c > 4096 * 256 and r % 41 == 0
    x, scale, zp, eq, edq = _draw(7, qtype, mode, r, c, group)
    q = ops.quantize(dev(x), dev(scale), dev(zp), qtype, False, False, mode, group)
    assert same_bytes(host(q), eq)
    assert same_bytes(host(ops.dequantize(q, dev(scale), dev(zp), qtype, mode, group)), edq)


@pytest.mark.parametrize("mode,group", [("row", 1), ("group", 13)])
def test_rows_beyond_the_tile_grid_fall_back_to_the_generic_kernel(ops, mode, group):
    """ceil(R / 32) = 65536 > 65535 although C % 4 == 0 and everything is aligned.  R = 65535 * 32 + 1 = 13^2 * 12409: groups of
    g = 13 rows (its smallest divisor).  The result equals the oracle's, and equals what the first 65535 * 32 rows alone (the
    tile kernel's largest grid) and the last row alone give."""
    import torch
    r0, c, qtype = 65535 * 32, 4, "uint8"
    r = r0 + 1
    assert r % group == 0
    x, scale, zp, eq, edq = _draw(3, qtype, mode, r, c, group)
    xd, sd, zd = dev(x), dev(scale), dev(zp)
    q = ops.quantize(xd, sd, zd, qtype, False, False, mode, group)
    assert same_bytes(host(q), eq)
    dq = ops.dequantize(q, sd, zd, qtype, mode, group)
    assert same_bytes(host(dq), edq)
    # the same parameters addressed from the parts: the first r0 rows as they are, the last row from its own parameter row
    pidx = B.param_index(mode, r, group)
    first = r0 // group * pidx[1]
    q2, dq2 = torch.full_like(q, 99), torch.full_like(dq, 99.0)
    assert B.raw_quantize(xd, r0, c, c, sd, zd, pidx, qtype, q2) == 0
    assert B.raw_quantize(xd[r0:], 1, c, c, sd[first:], zd[first:], pidx, qtype, q2[r0:]) == 0
    assert B.raw_dequantize(q, r0, c, qtype, sd, zd, pidx, dq2, c) == 0
    assert B.raw_dequantize(q[r0:], 1, c, qtype, sd[first:], zd[first:], pidx, dq2[r0:], c) == 0
    assert torch.equal(q2, q) and torch.equal(dq2.view(torch.int32), dq.view(torch.int32))


@pytest.mark.parametrize("qtype", ["uint8", "int4"])
@pytest.mark.parametrize("mode,group", MODES)
def test_misaligned_bases_and_leading_dimensions_give_the_aligned_bytes(ops, qtype, mode, group):
    """64 x 256 is tile-eligible; a base 4 bytes (x, x_out) or 1 byte (q) off 16, or a leading dimension of 257, sends the call to
    the generic kernels for pointer / stride reasons only; 260 keeps it on the tile kernel.  All give the oracle's bytes, and every
    byte outside the payload keeps its sentinel."""
    import torch
    r, c = 64, 256
    x, scale, zp, eq, edq = _draw(11, qtype, mode, r, c, group)
    sd, zd, pidx = dev(scale), dev(zp), B.param_index(mode, r, group)
    assert same_bytes(host(ops.quantize(dev(x), sd, zd, qtype, False, False, mode, group)), eq)
    assert same_bytes(host(ops.dequantize(dev(eq), sd, zd, qtype, mode, group)), edq)
    for ld, x_off, q_off in [(256, 1, 0), (256, 0, 1), (256, 1, 1), (260, 0, 0), (257, 0, 0), (260, 1, 0), (260, 0, 1)]:
        label = f"ld={ld} fp32 base +{x_off} byte base +{q_off}"
        xv, _ = B.strided(x, ld, x_off, fill=1e30)
        qbuf = torch.full((q_off + r * c + 16,), B.SENTINEL_U8, dtype=torch.uint8, device="cuda")
        qv = qbuf[q_off:q_off + r * c]
        assert xv.data_ptr() % 16 == 4 * x_off and qv.data_ptr() % 16 == q_off
        assert B.raw_quantize(xv, r, c, ld, sd, zd, pidx, qtype, qv) == 0, label
        assert host(qv).tobytes() == eq.tobytes(), label
        rest = torch.cat([qbuf[:q_off], qbuf[q_off + r * c:]])
        assert bool((rest == B.SENTINEL_U8).all()), label
        # K2 the other way round: bytes at qv, fp32 out with leading dimension ld at an offset of x_off elements
        obuf = torch.full((x_off + r * ld,), float(B.SENTINEL_F32), device="cuda")
        ov = obuf[x_off:x_off + r * ld].view(r, ld)
        assert B.raw_dequantize(qv, r, c, qtype, sd, zd, pidx, ov, ld) == 0, label
        assert same_bytes(host(ov[:, :c]), edq), label
        assert bool((ov[:, c:] == float(B.SENTINEL_F32)).all()) and bool((obuf[:x_off] == float(B.SENTINEL_F32)).all()), label
    # the same views through the Python front (it keeps a row stride and a base offset)
    xv, _ = B.strided(x, 257, 1, fill=1e30)
    assert same_bytes(host(ops.quantize(xv, sd, zd, qtype, False, False, mode, group)), eq)


@pytest.mark.parametrize("arm,r,c,ldo,qtype,float_zp", [("tile", 64, 256, 260, "uint8", False), ("tile", 33, 8, 12, "int8", False),
                                                        ("generic", 37, 63, 70, "int8", False), ("generic", 64, 256, 257, "uint4", False),
                                                        ("fzp", 64, 256, 260, "uint4", True), ("fzp", 37, 63, 64, "int8", True)])
@pytest.mark.parametrize("mode,group", [("row", 1), ("col", 1)])
def test_dequantize_strided_store(ops, arm, r, c, ldo, qtype, float_zp, mode, group):
    """ldo > C through the C ABI (`ops.dequantize` always passes C): the tile kernel's store, the generic kernel's, and
    oq_dequantize_fzp_f32's.  The gap columns keep a sentinel, the payload equals the oracle's and the contiguous call's."""
    import torch
    rng = np.random.default_rng(r * ldo)
    qmin, qmax = O.qrange(qtype, False, False)
    q = rng.integers(qmin, qmax + 1, size=(r, c)).astype(O.container_dtype(qtype))
    n = B.param_count(mode, r, c, group)
    scale = rng.uniform(0.01, 0.3, size=n).astype(np.float32)
    zp = rng.uniform(qmin - 2, qmax + 2, size=n).astype(np.float32) if float_zp else rng.integers(qmin, qmax + 1, size=n).astype(np.int32)
    expected = O.dequantize(q, B.expand(mode, r, c, group, scale), B.expand(mode, r, c, group, zp))
    qd, sd, zd = dev(q), dev(scale), dev(zp)
    assert same_bytes(host(ops.dequantize(qd, sd, zd, qtype, mode, group)), expected)
    out = torch.full((r, ldo), float(B.SENTINEL_F32), device="cuda")
    assert B.raw_dequantize(qd, r, c, qtype, sd, zd, B.param_index(mode, r, group), out, ldo) == 0
    assert same_bytes(host(out[:, :c]), expected)
    assert bool((out[:, c:] == float(B.SENTINEL_F32)).all())


@pytest.mark.parametrize("mode,group", MODES)
def test_dequantize_float_zero_points_signed_container(ops, mode, group):
    """oq_dequantize_fzp_f32 with int8 values (negative ones included) and negative float zero points: (f32(q) - zp) * s."""
    r, c = 48, 36
    rng = np.random.default_rng(21)
    q = rng.integers(-128, 128, size=(r, c)).astype(np.int8)
    q[0, :4] = [-128, -1, 0, 127]
    n = B.param_count(mode, r, c, group)
    scale = rng.uniform(0.01, 0.3, size=n).astype(np.float32)
    zp = rng.uniform(-130.0, 10.0, size=n).astype(np.float32)
    zp[0] = -3.4
    expected = (q.astype(np.float32) - B.expand(mode, r, c, group, zp)) * B.expand(mode, r, c, group, scale)
    assert (zp < 0).any() and (q < 0).any()
    assert same_bytes(host(ops.dequantize(dev(q), dev(scale), dev(zp), "int8", mode, group)), expected)
    truncated = (q.astype(np.float32) - np.trunc(B.expand(mode, r, c, group, zp))) * B.expand(mode, r, c, group, scale)
    assert not np.array_equal(truncated, expected)


@pytest.mark.parametrize("qtype", BYTE_TYPES)
@pytest.mark.parametrize("scale", [0.125, 0.1], ids=["exact_ties", "tenth"])
@pytest.mark.parametrize("cols", [4, 3], ids=["tile", "generic"])
def test_ties_and_range_ends(ops, qtype, scale, cols):
    """x = (k + 0.5) s and k s for every k from below qmin - zp to above qmax - zp: with s = 2^-3 every quotient is an exact tie
    (half to even, not half up / away / truncation), with s = 0.1f none is exact and the fp32 division decides; both ends clamp."""
    qmin, qmax = O.qrange(qtype, False, False)
    s = np.float32(scale)
    for zp in (qmin, qmin + (qmax - qmin) // 3, qmax):
        k = np.arange(qmin - zp - 3, qmax - zp + 4).astype(np.float32)
        x = np.concatenate([(k + np.float32(0.5)) * s, k * s, (k - np.float32(0.5)) * s])
        x = np.concatenate([x, np.zeros(-x.size % 12, np.float32)]).reshape(-1, cols)
        expected = O.quantize(x, s, np.int32(zp), qtype, False, False)
        if scale == 0.125:                                                # the ties are exact: odd multiples of one half
            assert np.count_nonzero(((x / s) * 2) % 2 == 1) >= 2 * (qmax - qmin)
        assert expected.min() == qmin and expected.max() == qmax
        got = ops.quantize(dev(x), dev(np.array([s])), dev(np.array([zp], np.int32)), qtype, False, False, "tensor")
        assert same_bytes(host(got), expected), f"zp={zp}"


# ============================================================================= 3. 32-bit containers
_I32_VALUES = [0, 1, -1, 2**24 + 1, -(2**24 + 1), B.INT32_MIN, B.INT32_MAX, 123456789, -2**30]
_U32_VALUES = [0, 1, 2**24 + 1, 2**31 - 1, 2**31, 2**31 + 129, 2**32 - 1, 123456789]


@pytest.mark.parametrize("qtype,values", [("int32", _I32_VALUES), ("uint32", _U32_VALUES)])
def test_dequantize_32_bit_containers(ops, qtype, values):
    """(q.astype(f32) - zp.astype(f32)) * s with integers and zero points at the ends of the type and at 2^24 + 1, where the
    conversion to fp32 rounds.  A uint32 zero point of 2^31 or more is read as unsigned (include/oq_hip.h), whether it arrives as
    a uint32 tensor, as an int64 tensor or as its int32 bits."""
    import torch
    dt = O.container_dtype(qtype)
    zp = np.array(values, dt)
    q = np.repeat(np.array(values, dt)[None, :], zp.size, 0)              # row i: every value against zero point i
    scale = np.resize(np.array([1.0, 0.5, 3.0, 0.1], np.float32), zp.size)
    expected = (q.astype(np.float32) - zp.astype(np.float32)[:, None]) * scale[:, None]
    assert expected.dtype == np.float32
    qd, sd = dev(q), dev(scale)
    assert qd.dtype == ops.container_dtype(qtype)
    for zd in (dev(zp), dev(zp.astype(np.int64)), dev(zp.view(np.int32))):
        assert same_bytes(host(ops.dequantize(qd, sd, zd, qtype, "row")), expected), zd.dtype
    out = torch.full((zp.size, q.shape[1] + 3), float(B.SENTINEL_F32), device="cuda")      # and the strided store of this arm
    assert B.raw_dequantize(qd, *q.shape, qtype, sd, dev(zp.view(np.int32)), (1, 1, 0), out, out.shape[1]) == 0
    assert same_bytes(host(out[:, :q.shape[1]]), expected) and bool((out[:, q.shape[1]:] == float(B.SENTINEL_F32)).all())


@pytest.mark.parametrize("qtype,symmetric,reduce_range", [("int32", False, False), ("int32", True, False), ("int32", False, True),
                                                          ("uint32", False, False), ("uint32", False, True)])
def test_quantize_32_bit_containers(ops, qtype, symmetric, reduce_range):
    """clip(int32(rint(x / s)) + zp) with the sum in int64, as NumPy evaluates it for uint32 zero points: sums that stay inside
    int32, and sums that leave it while rint(x / s) does not -- those must clamp, not wrap.  The clamp range is oq_qrange's."""
    qmin, qmax = O.qrange(qtype, symmetric, reduce_range)
    assert B.L.qrange(B.L.QTYPE_CODE[qtype], symmetric, reduce_range) == (qmin, qmax)
    top = 2.0**31 - 128                                                    # the largest fp32 below 2^31
    quotients = np.array([0, 1.5, 2.5, -0.5, -1.5, 1000, -1000, 2**24 + 2, 2.0**30, -(2.0**30), 2.0**30 + 128, top, -top, -(2.0**31)], np.float32)
    if qtype == "int32":
        zps = np.array([0, 5, -5, 1000, -1000, 2**30, -2**30, B.INT32_MAX, B.INT32_MIN], np.int64)
    else:
        zps = np.array([0, 5, 1000, 2**31 - 1, 2**31, 2**31 + 1000, 2**32 - 1], np.int64).astype(np.uint32)
    scale = np.resize(np.array([1.0, 0.5, 2.0], np.float32), zps.size)
    x = quotients[None, :] * scale[:, None]                               # powers of two: x / s is the quotient again, exactly
    expected = O.quantize(x, scale[:, None], zps[:, None], qtype, symmetric, reduce_range)
    rint = np.rint(quotients).astype(np.int64)
    exact = np.clip(rint[None, :] + zps.astype(np.int64)[:, None], qmin, qmax)
    assert np.array_equal(expected.astype(np.int64), exact)               # NumPy did not wrap either: these ARE the int64 sums
    sums = rint[None, :] + zps.astype(np.int64)[:, None]
    assert ((sums > B.INT32_MAX) | (sums < B.INT32_MIN)).any() and ((sums <= B.INT32_MAX) & (sums >= B.INT32_MIN)).any()
    for zd in ((dev(zps),) if qtype == "int32" else (dev(zps), dev(zps.astype(np.int64)), dev(zps.view(np.int32)))):
        got = ops.quantize(dev(x), dev(scale), zd, qtype, symmetric, reduce_range, "row")
        assert same_bytes(host(got), expected), zd.dtype


def test_functional_mirror_on_32_bit_zero_points():
    """`functional` takes host arrays, so it can look at the values: a uint32 zero point of 2^31 or more passes as it is, one
    outside the range the kernels read (unsigned for uint32, int32 otherwise) is a ValueError that names the zero point."""
    from onnx_quantize_amd import QuantType
    from onnx_quantize_amd.algorithms import functional as F
    q = np.array([[0, 5, 2**31, 2**32 - 1]], np.uint32)
    zp = np.array([2**31 + 7], np.uint32)
    s = np.array([0.5], np.float32)
    got = F._dequantize_array(q, s, zp)
    assert same_bytes(got, (q.astype(np.float32) - zp.astype(np.float32)) * s)
    x = np.array([[-8.0, 0.0, 9.0, 2.0**29]], np.float32)
    expected = O.quantize(x, s, zp, "uint32", False, False)
    assert same_bytes(F._quantize_array_from_qparams(x, s, zp, QuantType.QUInt32, False, False), expected)
    with pytest.raises(ValueError, match="zero point"):
        F._dequantize_array(q, s, np.array([2**32], np.int64))
    with pytest.raises(ValueError, match="zero point"):
        F._dequantize_array(q, s, np.array([-1], np.int64))
    with pytest.raises(ValueError, match="zero point"):
        F._dequantize_array(q.view(np.int32), s, np.array([2**31], np.int64))
    with pytest.raises(ValueError, match="zero point"):
        F._quantize_array_from_qparams(x, s, np.array([2**32], np.int64), QuantType.QUInt32, False, False)


# ============================================================================= 4. where NumPy's cast is not defined
_ZERO_POINTS = {"int8": (5, 0, -7), "uint8": (130, 0, -3), "int4": (3, 0, -2), "uint4": (9, 0, -1)}


@pytest.mark.parametrize("qtype", BYTE_TYPES)
@pytest.mark.parametrize("cols", [8, 7], ids=["tile", "generic"])
def test_quantize_where_numpy_is_undefined(ops, qtype, cols):
    """x / s = NaN, +-inf, +-2^31, +-3e9 with a positive, a zero and a negative zero point: the rule of include/oq_hip.h --
    overflow lands on the end of the range it left through, NaN on clamp(zp), whatever the sign of zp (the module docstring holds
    NumPy's values beside these)."""
    qmin, qmax = O.qrange(qtype, False, False)
    zps = np.array(_ZERO_POINTS[qtype], np.int32)
    for s in (np.float32(1.0), np.float32(0.5)):
        quotients = np.concatenate([B.SPECIAL_QUOTIENTS, np.float32([6.5])])[:cols]       # the tile arm carries one ordinary value
        x = np.repeat((quotients * s)[None, :], zps.size, 0)
        assert np.array_equal(B.quiet(np.divide, x, s)[0], quotients, equal_nan=True)
        got = host(ops.quantize(dev(x), dev(np.full(zps.size, s)), dev(zps), qtype, False, False, "row")).astype(np.int64)
        assert np.array_equal(got, B.k1_rule(x, np.full_like(x, s), np.repeat(zps[:, None], cols, 1), qmin, qmax))
        # ... and the rule spelled out: NaN, +inf, -inf, +2^31, -2^31, +3e9, -3e9
        for row, zp in zip(got, zps):
            assert row[:7].tolist() == [min(max(int(zp), qmin), qmax), qmax, qmin, qmax, qmin, qmax, qmin], (qtype, zp)


def test_bias_where_numpy_is_undefined(ops):
    """oq_quantize_bias_f32: a quotient outside int32 saturates, NaN gives 0, a zero scale included (bias / 0 = +-inf, 0 / 0 = NaN)."""
    lo, hi = B.INT32_MIN, B.INT32_MAX
    for s in (np.float32(1.0), np.float32(0.25)):
        q, bs = ops.quantize_bias(dev(B.SPECIAL_QUOTIENTS * s), 1.0, dev(np.array([s])))
        assert host(q).tolist() == [0, hi, lo, hi, lo, hi, lo] and same_bytes(host(bs), np.full(7, s))
    q, bs = ops.quantize_bias(dev(np.array([1.0, -1.0, 0.0], np.float32)), 0.0, dev(np.array([0.5], np.float32)))
    assert host(q).tolist() == [hi, lo, 0] and same_bytes(host(bs), np.zeros(3, np.float32))
    q, _ = ops.quantize_bias(dev(np.array([1.0, -1.0, 0.0, 2.0], np.float32)), 1.0, dev(np.array([0.0, 0.0, 0.0, 0.5], np.float32)))
    assert host(q).tolist() == [hi, lo, 0, 4]


# ============================================================================= 5. oq_qparams_f32 / oq_qparams_f64
_GRIDS = [(qtype, sym, rr) for qtype in BYTE_TYPES for sym in (False, True) for rr in (False, True)]


def _expected_qparams(lo, hi, qtype, sym, rr):
    scale, wide = B.quiet(O.qparams, lo, hi, qtype, sym, rr, np.float32, np.float64)       # the zero point before any integer cast
    _, narrow = B.quiet(O.qparams, lo, hi, qtype, sym, rr, np.float32)
    return scale, wide, narrow


@pytest.mark.parametrize("count", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_qparams_against_the_oracle(ops, dtype, count):
    """Scale bytes and zero points of oq_qparams_f32 / _f64 on every 1-byte grid: (0, 0), scales just below / at / just above
    `tiny` (FLT_MIN resp. DBL_MIN), subnormal, infinite and NaN ends, ranges that do not hold zero, lo > hi; one block, a full
    block, a second block (test_building_block_cases.py checks on the host that the ranges reach all of that on every grid).
    Where the oracle's scale is NaN the kernel's must be NaN (payloads are not compared)."""
    fn = ops.qparams if dtype is np.float32 else ops.qparams_f64
    for qtype, sym, rr in _GRIDS:
        lo, hi = B.qparams_ranges(dtype, qtype, sym, rr, count)
        e_scale, e_wide, e_narrow = _expected_qparams(lo, hi, qtype, sym, rr)
        scale, zp = (host(t) for t in fn(dev(lo), dev(hi), qtype, sym, rr))
        label = f"{qtype} sym={sym} rr={rr}"
        assert scale.dtype == np.float32 and zp.dtype == np.int32
        nan = np.isnan(e_scale)
        assert np.array_equal(np.isnan(scale), nan), label
        bad = np.flatnonzero(scale[~nan].view(np.uint32) != e_scale[~nan].view(np.uint32))
        assert bad.size == 0, (label, lo[~nan][bad][:4], hi[~nan][bad][:4], scale[~nan][bad][:4], e_scale[~nan][bad][:4])
        assert np.array_equal(B.narrowed(zp, qtype), e_narrow), label
        defined = ~np.isnan(e_wide)                                        # elsewhere the oracle itself casts NaN to an integer
        assert np.array_equal(zp[defined], e_wide[defined].astype(np.int32)), label


def test_qparams_front_takes_any_shape(ops):
    """`ops.qparams` on a non-contiguous [n, 1] view (what `MinMaxCalibrator.compute_qparams_many` may hand over)."""
    lo, hi = B.qparams_ranges(np.float32, "uint8", False, False, 300)
    both = dev(np.stack([lo, hi], axis=1))
    rmin, rmax = both[:, 0:1], both[:, 1:2]
    assert not rmin.is_contiguous() and rmin.shape == (300, 1)
    scale, zp = ops.qparams(rmin, rmax, "uint8", False, False)
    e_scale, _, e_narrow = _expected_qparams(lo, hi, "uint8", False, False)
    assert scale.shape == (300, 1) and zp.shape == (300, 1)
    ok = ~np.isnan(e_scale)
    assert same_bytes(host(scale).reshape(-1)[ok], e_scale[ok]) and np.array_equal(B.narrowed(host(zp).reshape(-1), "uint8"), e_narrow)


# ============================================================================= 6. oq_quantize_bias_f32
@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("per_channel", [False, True])
def test_bias_ties_and_rounded_scale_products(ops, n, per_channel):
    """Exact ties bias = (k + 0.5) s with power-of-two scales (half to even), and an x_scale whose fp32 product with w_scale rounds:
    bias_scale_out is np.float32 multiplication, bit for bit."""
    rng = np.random.default_rng(n + per_channel)
    n_w = n if per_channel else 1
    w_scale = np.float32(2.0) ** rng.integers(-9, -2, size=n_w).astype(np.float32)
    x_scale = np.float32(0.25)
    k = rng.integers(-100000, 100000, size=n).astype(np.float32)
    k[0] = 2.0**23 - 1                                                     # the largest k whose k + 0.5 is an fp32
    bias = (k + np.float32(0.5)) * (w_scale * x_scale)
    eq, es, _ = O.quantize_bias(bias, x_scale, w_scale)
    assert np.array_equal(eq, np.where(k % 2 == 0, k, k + 1).astype(np.int32))                          # k + 0.5 -> the even neighbour
    q, bs = ops.quantize_bias(dev(bias), float(x_scale), dev(w_scale))
    assert same_bytes(host(q), eq) and same_bytes(host(bs), np.broadcast_to(es, (n,)))
    # a product that rounds
    w_scale = rng.uniform(0.001, 0.2, size=n_w).astype(np.float32)
    x_scale = np.float32(0.1)
    assert np.any(w_scale.astype(np.float64) * np.float64(x_scale) != (w_scale * x_scale).astype(np.float64))
    bias = (rng.standard_normal(n) * 4).astype(np.float32)
    eq, es, _ = O.quantize_bias(bias, x_scale, w_scale)
    q, bs = ops.quantize_bias(dev(bias), float(x_scale), dev(w_scale))
    assert same_bytes(host(q), eq) and same_bytes(host(bs), np.broadcast_to(es, (n,)))


def test_bias_refuses_a_scale_count_that_is_neither_1_nor_n():
    import torch
    bias, w = dev(np.ones(5, np.float32)), dev(np.ones(5, np.float32))
    q = torch.full((5,), 77, dtype=torch.int32, device="cuda")
    bs = torch.full((5,), float(B.SENTINEL_F32), device="cuda")
    for n_w in (2, 4, 6, 0):
        st = B.L.load().oq_quantize_bias_f32(bias.data_ptr(), 5, w.data_ptr(), n_w, 1.0, q.data_ptr(), bs.data_ptr(), B.stream())
        assert st == B.L.OQ_ERR_INVALID_ARGUMENT, n_w
    torch.cuda.synchronize()
    assert bool((q == 77).all()) and bool((bs == float(B.SENTINEL_F32)).all())


# ============================================================================= 7. the packers, against NumPy only
def _nibble_pairs(values):
    flat = np.asarray(values).reshape(-1).view(np.uint8) & 0x0F
    flat = np.concatenate([flat, np.zeros(flat.size % 2, np.uint8)])       # _pack.py:15-17: zero pad
    return (flat[0::2] | (flat[1::2] << 4)).astype(np.uint8)


@pytest.mark.parametrize("count", [1, 2, 15, 16, 17, 31, 32, 33, 47, 4096, 4101])
@pytest.mark.parametrize("dtype", [np.int8, np.uint8], ids=["int8", "uint8"])
def test_pack_nibbles(ops, count, dtype):
    """The 16-values-per-thread arm (aligned calls, count >= 16) and the one-byte-per-thread arm (ragged end, misaligned source or
    destination) against NumPy: negative int8 values leave no sign bits in the neighbour nibble, garbage in the high nibble of a
    uint8 is masked, and no byte of `out` behind (count + 1) / 2 is written."""
    import torch
    rng = np.random.default_rng(count)
    v = rng.integers(-8, 8, size=count).astype(np.int8) if dtype is np.int8 else rng.integers(0, 256, size=count).astype(np.uint8)
    v[0] = -8 if dtype is np.int8 else 0xF7
    expected = _nibble_pairs(v)
    nbytes = (count + 1) // 2
    assert same_bytes(host(ops.pack_nibbles(dev(v))), expected)
    for src_off, dst_off in [(0, 0), (1, 0), (0, 1), (16, 8), (0, 4)]:
        src = torch.full((src_off + count,), 0x5A, dtype=torch.uint8, device="cuda")
        src[src_off:] = dev(v.view(np.uint8))
        out = torch.full((dst_off + nbytes + 16,), B.SENTINEL_U8, dtype=torch.uint8, device="cuda")
        st = B.L.load().oq_pack_nibbles(src[src_off:].data_ptr(), count, out[dst_off:].data_ptr(), B.stream())
        assert st == 0
        got = host(out)
        assert got[dst_off:dst_off + nbytes].tobytes() == expected.tobytes(), (src_off, dst_off)
        assert np.all(got[:dst_off] == B.SENTINEL_U8) and np.all(got[dst_off + nbytes:] == B.SENTINEL_U8), (src_off, dst_off)


@pytest.mark.parametrize("n,blocks", [(1, 1), (1, 2), (3, 1), (5, 7), (64, 8), (257, 3)])
def test_pack_zero_points_u4(ops, n, blocks):
    """_common.py:96-121: [N, ceil(blocks / 2)], even block in the low nibble, pad nibble 8 on odd `blocks`, high nibbles masked."""
    zp = np.random.default_rng(n * 10 + blocks).integers(0, 256, size=(n, blocks)).astype(np.uint8)
    padded = np.concatenate([zp & 0x0F, np.full((n, blocks % 2), 8, np.uint8)], axis=1)
    expected = (padded[:, 0::2] | (padded[:, 1::2] << 4)).astype(np.uint8)
    assert (zp > 15).any() or n * blocks < 4
    assert same_bytes(host(ops.pack_zero_points_u4(dev(zp.reshape(-1)), n, blocks)), expected)
    if blocks > 1:                                                         # the oracle packs only then (and does not mask: feed it nibbles)
        assert np.array_equal(O.matmul_nbits_layout(np.zeros((2 * blocks, n), np.uint8), np.zeros(n * blocks), zp & 0x0F, 2, 4)[2], expected)


@pytest.mark.parametrize("k,n,g,bits", [(2, 1, 2, 4), (192, 5, 96, 4), (192, 70, 96, 8), (128, 65, 128, 4), (66, 64, 2, 8), (320, 129, 64, 4)])
def test_pack_matmul_nbits(ops, k, n, g, bits):
    """The blob [N, K/g, g*bits/8] against `matmul_nbits_layout`: a group boundary inside a 64-row tile that neither divides nor is
    a multiple of 64 (g = 96), g = 2, a last tile of 2 rows (K = 66) and of 1 column (N = 65, 129)."""
    q = np.random.default_rng(k + n).integers(0, 1 << bits, size=(k, n)).astype(np.uint8)
    expected = O.matmul_nbits_layout(q, np.zeros(n * (k // g), np.float32), np.zeros(n * (k // g), np.uint8), g, bits)[0]
    assert expected.shape == (n, k // g, g * bits // 8)
    assert same_bytes(host(ops.pack_matmul_nbits(dev(q), g, bits)), expected)
    if bits == 4:                                                          # garbage above the nibble is masked
        assert same_bytes(host(ops.pack_matmul_nbits(dev(q | 0xA0), g, bits)), expected)


@pytest.mark.parametrize("k,g,bits,status", [(6, 3, 4, "OQ_ERR_INVALID_ARGUMENT"), (6, 4, 4, "OQ_ERR_INVALID_ARGUMENT"), (6, 0, 8, "OQ_ERR_INVALID_ARGUMENT"),
                                             (8, 4, 5, "OQ_ERR_UNSUPPORTED")])
def test_pack_matmul_nbits_refusals(k, g, bits, status):
    """Odd g, K % g != 0, bits = 5: the status, and an untouched output."""
    import torch
    q = torch.zeros((k, 4), dtype=torch.uint8, device="cuda")
    out = torch.full((64,), B.SENTINEL_U8, dtype=torch.uint8, device="cuda")
    assert B.L.load().oq_pack_matmul_nbits(q.data_ptr(), k, 4, g, bits, out.data_ptr(), B.stream()) == getattr(B.L, status)
    torch.cuda.synchronize()
    assert bool((out == B.SENTINEL_U8).all())
