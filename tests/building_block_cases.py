"""What the tests of the small kernels share (test_building_blocks_gpu.py): csrc/elementwise.hip and `minmax_rows` of csrc/reduce.hip.

Every expectation is NumPy's: the oracle's restatement (`oq_oracle.quantize`, `dequantize`, `qparams`, `quantize_bias`,
`matmul_nbits_layout`) or a few lines of NumPy here.  Nothing in this file runs a kernel to obtain an expectation.

`dev` / `host`       NumPy <-> device; uint32 arrays travel as their int32 bits and are re-viewed on the other side.
`strided`            a [rows, cols] device view with a leading dimension and a base offset of the caller's choice, its gaps filled.
`param_index` ...    the four parameter modes of oq_quantize_f32 / oq_dequantize_f32 and their NumPy expansion.
`raw_*`              the C ABI itself, for what the Python front never passes: ldo > C, misaligned bases, status codes.
`k1_rule`            the header's rule for oq_quantize_f32 where NumPy's cast is undefined, in Python integers.
`qparams_ranges`     the (lo, hi) ranges of section 5, per grid and dtype.
"""
import warnings

import numpy as np
import torch

import oq_oracle as O
from onnx_quantize_amd.hip import _lib as L

BYTE_TYPES = ["int4", "uint4", "int8", "uint8"]
MODES = [("tensor", 1), ("row", 1), ("col", 1), ("group", 16)]
INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1
SENTINEL_F32 = np.float32(-7.7701e22)
SENTINEL_U8 = 0xA5


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda().view(torch.uint32)
    return torch.from_numpy(a).cuda()


def host(t):
    if t.dtype == torch.uint32:
        return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
    return t.cpu().numpy()


def stream():
    return torch.cuda.current_stream().cuda_stream


def quiet(fn, *args, **kw):
    """NumPy on ranges and casts it warns about (NaN / inf arithmetic, undefined float -> integer casts)."""
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*args, **kw)


def strided(a, ld, offset=0, fill=0):
    """`a` [rows, cols] on the device as a view with leading dimension `ld` whose first element sits `offset` elements behind
    the start of a fresh allocation; everything outside the view holds `fill`.  Returns (view, the whole flat buffer)."""
    a = np.ascontiguousarray(a)
    rows, cols = a.shape
    assert ld >= cols and offset >= 0
    buf = torch.full((offset + rows * ld,), fill, dtype=torch.from_numpy(a[:1, :1].copy()).dtype, device="cuda")
    view = buf[offset:offset + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(dev(a))
    return view, buf


# ----------------------------------------------------------------------------- parameter modes of K1 / K2
def param_count(mode, r, c, group):
    return {"tensor": 1, "row": r, "col": c, "group": (r // group) * c}[mode]


def param_index(mode, r, group):
    """(row_div, row_stride, col_stride) of include/oq_hip.h."""
    return {"tensor": (1, 0, 0), "row": (1, 1, 0), "col": (1, 0, 1), "group": (group, 1, r // group)}[mode]


def expand(mode, r, c, group, values):
    """The [r, c] array of the parameter each element uses."""
    values = np.asarray(values).reshape(-1)
    if mode == "tensor":
        return np.full((r, c), values[0], values.dtype)
    if mode == "row":
        return np.repeat(values[:, None], c, 1)
    if mode == "col":
        return np.repeat(values[None, :], r, 0)
    return values[np.arange(c)[None, :] * (r // group) + (np.arange(r) // group)[:, None]]      # entry n * (R / g) + kg


def draw_params(rng, qtype, count, symmetric=False, reduce_range=False):
    qmin, qmax = O.qrange(qtype, symmetric, reduce_range)
    return rng.uniform(0.01, 0.3, size=count).astype(np.float32), rng.integers(qmin, qmax + 1, size=count).astype(np.int32)


# ----------------------------------------------------------------------------- the C ABI
def raw_quantize(x, r, c, ldx, scale, zp, pidx, qtype, q, symmetric=False, reduce_range=False):
    return L.load().oq_quantize_f32(x.data_ptr(), r, c, ldx, scale.data_ptr(), zp.data_ptr(), *pidx, L.QTYPE_CODE[qtype],
                                    int(symmetric), int(reduce_range), q.data_ptr(), stream())


def raw_dequantize(q, r, c, qtype, scale, zp, pidx, out, ldo):
    fn = L.load().oq_dequantize_fzp_f32 if zp.dtype.is_floating_point else L.load().oq_dequantize_f32
    return fn(q.data_ptr(), r, c, L.QTYPE_CODE[qtype], scale.data_ptr(), zp.data_ptr(), *pidx, out.data_ptr(), ldo, stream())


# ----------------------------------------------------------------------------- section 4: the documented rule of K1
SPECIAL_QUOTIENTS = np.array([np.nan, np.inf, -np.inf, 2.0**31, -(2.0**31), 3e9, -3e9], np.float32)


def sat32(quotient) -> int:
    """include/oq_hip.h: saturates to [-2^31, 2^31 - 1], NaN -> 0; rint (half to even) inside."""
    quotient = float(quotient)
    if quotient != quotient:
        return 0
    if quotient >= 2.0**31:
        return INT32_MAX
    if quotient < -(2.0**31):
        return INT32_MIN
    return int(np.rint(quotient))


def k1_rule(x, scale, zp, qmin, qmax):
    """q = clamp(sat32(rint(x / scale)) + zp, qmin, qmax), the sum in Python integers; x, scale, zp of one shape."""
    quotient = quiet(np.divide, np.asarray(x, np.float32), np.asarray(scale, np.float32))
    out = [min(max(sat32(t) + int(z), qmin), qmax) for t, z in zip(quotient.reshape(-1), np.asarray(zp).reshape(-1))]
    return np.array(out, np.int64).reshape(quotient.shape)


# ----------------------------------------------------------------------------- section 5: ranges for Q1
def grid_span(qtype, symmetric, reduce_range):
    """What the range is divided by: qmax - qmin, or the symmetric `levels` of utils.py:273-298."""
    qmin, qmax = O.qrange(qtype, symmetric, reduce_range)
    if not symmetric:
        return float(qmax - qmin)
    zero = np.round((qmax + qmin) / 2.0)
    return float(min(qmax - zero, zero - qmin))


def qparams_ranges(dtype, qtype, symmetric, reduce_range, count, seed=0):
    """`count` (lo, hi) pairs of `dtype`: the edge cases first, as many as fit (every count of 255 and more holds them all; a
    smaller one starts at an index of its own), ordinary ranges behind them."""
    dtype = np.dtype(dtype).type
    tiny, span = dtype(np.finfo(dtype).tiny), dtype(grid_span(qtype, symmetric, reduce_range))
    pairs = [(0.0, 0.0), (-0.0, 0.0)]
    at = tiny * span                                              # the range whose scale is (about) `tiny`
    for steps in range(-3, 4):                                    # ... and its neighbours on both sides, one-sided and two-sided
        v = at
        for _ in range(abs(steps)):
            v = np.nextafter(v, dtype(np.inf if steps > 0 else 0))
        pairs += [(0.0, v), (-v, 0.0), (-v / dtype(2), v / dtype(2)), (-v, v)]
    sub = dtype(np.finfo(dtype).smallest_subnormal)
    pairs += [(-sub, sub), (0.0, sub * dtype(1000)), (-tiny / dtype(4), tiny / dtype(8))]                       # subnormal ranges
    pairs += [(-1.0, np.inf), (-np.inf, 1.0), (-np.inf, np.inf), (0.0, np.inf),                                 # infinite ends
              (np.nan, 1.0), (-1.0, np.nan), (np.nan, np.nan),                                                  # NaN in either end
              (1.0, 3.0), (-3.0, -1.0), (0.25, 0.5), (2.0, 1.0),                                                # zero not inside; lo > hi
              (-1.5, 2.5), (-0.001, 1000.0), (-6.0, 0.0), (0.0, 6.0)]
    if dtype is np.float64:                                       # double scales that are normal but whose fp32 cast is not
        for s in (1e-40, 1.5e-45, 0.7e-45, 1e-46, 1e-50, 1e-300, 1e39, 1e300):
            pairs += [(-s * float(span) / 2, s * float(span) / 2), (0.0, s * float(span))]
    rng = np.random.default_rng(seed + count)
    lo = -np.abs(rng.standard_normal(count)) * rng.choice([1e-3, 1.0, 50.0], size=count)
    hi = np.abs(rng.standard_normal(count)) * rng.choice([1e-3, 1.0, 50.0], size=count)
    lo, hi = lo.astype(dtype), hi.astype(dtype)
    n = min(count, len(pairs))
    start = (count * 7) % len(pairs) if count < len(pairs) else 0   # small counts still see different edge cases
    for i in range(n):
        lo[i], hi[i] = pairs[(start + i) % len(pairs)]
    return lo, hi


def narrowed(zp, qtype):
    """A zero point as `_compute_qparams` returns it: narrowed to the container dtype."""
    return quiet(np.asarray, zp, dtype=O.container_dtype(qtype))
