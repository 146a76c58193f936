"""The helpers the tests of the small kernels stand on (tests/building_block_cases.py), checked on the host.  No kernel is launched."""
import numpy as np
import pytest

import oq_oracle as O
import building_block_cases as B

GRIDS = [(qtype, sym, rr) for qtype in B.BYTE_TYPES for sym in (False, True) for rr in (False, True)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_qparams_ranges_reach_both_sides_of_tiny(dtype):
    """On every grid the ranges give the oracle a scale just above `tiny`, one exactly at it where the division allows, and the
    switch to 1; NaN and infinite scales; the float64 set holds double scales that are normal while their fp32 cast is
    subnormal, zero or infinite."""
    tiny = np.finfo(dtype).tiny
    for qtype, sym, rr in GRIDS:
        lo, hi = B.qparams_ranges(dtype, qtype, sym, rr, 255)
        raw = B.quiet(O.qparams, lo, hi, qtype, sym, rr, dtype)[0]
        label = (qtype, sym, rr)
        assert (raw == 1).sum() >= 8 and ((raw >= tiny) & (raw <= tiny * (1 + 1e-5))).any(), label
        assert np.isinf(raw).any() and np.isnan(raw).any(), label
        if dtype is np.float64:
            cast = B.quiet(raw.astype, np.float32)
            sub = np.finfo(np.float32).tiny
            assert ((cast > 0) & (cast < sub)).any() and ((cast == 0) & (raw > 0)).any() and (np.isinf(cast) & np.isfinite(raw)).any(), label
    first = [B.qparams_ranges(dtype, "uint8", False, False, n) for n in (1, 255, 256, 257, 1000)]
    assert [lo.size for lo, _ in first] == [1, 255, 256, 257, 1000] and all(lo.dtype == dtype and hi.dtype == dtype for lo, hi in first)


@pytest.mark.parametrize("qtype", B.BYTE_TYPES)
def test_k1_rule_is_numpy_where_numpy_is_defined(qtype):
    """The header's rule restated in Python integers equals `oq_oracle.quantize` on ordinary values (ties included), and gives
    the table of test_building_blocks_gpu.py's docstring on the quotients NumPy cannot cast."""
    qmin, qmax = O.qrange(qtype, False, False)
    rng = np.random.default_rng(3)
    x = np.concatenate([(rng.standard_normal(500) * 40).astype(np.float32), (np.arange(-300, 300) + 0.5).astype(np.float32) * np.float32(0.25)])
    scale = np.full(x.shape, 0.25, np.float32)
    zp = rng.integers(qmin, qmax + 1, size=x.shape).astype(np.int32)
    assert np.array_equal(B.k1_rule(x, scale, zp, qmin, qmax), O.quantize(x, scale, zp, qtype, False, False).astype(np.int64))
    for z in (3, 0, -2):
        got = B.k1_rule(B.SPECIAL_QUOTIENTS, np.ones(7, np.float32), np.full(7, z), qmin, qmax).tolist()
        assert got == [min(max(z, qmin), qmax), qmax, qmin, qmax, qmin, qmax, qmin]


def test_expand_addresses_parameters_like_the_header():
    """include/oq_hip.h: entry (r / row_div) * row_stride + c * col_stride."""
    r, c, g = 6, 4, 2
    for mode, group in (("tensor", 1), ("row", 1), ("col", 1), ("group", g)):
        n = B.param_count(mode, r, c, group)
        rd, rs, cs = B.param_index(mode, r, group)
        values = np.arange(100, 100 + n)
        by_formula = np.array([[values[(i // rd) * rs + j * cs] for j in range(c)] for i in range(r)])
        assert np.array_equal(B.expand(mode, r, c, group, values), by_formula), mode
