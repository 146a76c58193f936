"""The pair build of the wave kernel (csrc/rtn.hip, `rtn_group_wave_pair`): 4-bit groups of 128 rows with an even
K / 128 run in blocks of two neighbouring k-groups x four strips, which exchange their finished bytes through LDS and store whole
128-byte lines of the MatMulNBits blob, 8-byte scale pairs and 2-byte zero-point pairs.  Only where and when a byte is stored
differs from the four-wave build, so everything is compared bit for bit with the oracle, at the smallest shapes that reach each
edge of the build, into output buffers with 256 bytes of 0xA5 on either side."""
import warnings

import numpy as np
import pytest

import oq_oracle as O

pytestmark = pytest.mark.gpu

G = 128
PAD = 256


@pytest.fixture(scope="module")
def ops():
    import torch
    from onnx_quantize_amd.hip import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def oracle(w, qtype, sym=False):
    """(blob [N, K/g, 64], scale [N*K/g, 1], zp [N*K/g, 1]) of the oracle: rtn_quantize + the blob packer."""
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eq, es, ez = O.rtn_quantize(w, qtype, "group", G, sym)
    u = (eq.astype(np.int16) & 0xF).astype(np.uint8)          # two's-complement nibbles
    return O.matmul_nbits_layout(u, es, ez, G, 4)[0], es, ez


def guarded(nbytes):
    import torch
    return torch.full((PAD + nbytes + PAD,), 0xA5, dtype=torch.uint8, device="cuda")


def quantize_guarded(ops, wd, qtype, sym=False):
    """ops.rtn_quantize into buffers that have PAD bytes of 0xA5 before and after: numpy (blob, scale, zp); the pads must stay."""
    k, n = wd.shape
    count = n * k // G
    bufs = guarded(n * k // 2), guarded(4 * count), guarded(count)
    import torch
    q = bufs[0][PAD:-PAD].view(n, k // G, G // 2)
    s = bufs[1][PAD:-PAD].view(torch.float32)
    z = bufs[2][PAD:-PAD].view(ops.container_dtype(qtype))
    q, s, z = ops.rtn_quantize(wd, qtype, "group", G, sym, layout="nbits", out=(q, s, z))
    for name, b in zip(("blob", "scale", "zero point"), bufs):
        h = b.cpu().numpy()
        assert (h[:PAD] == 0xA5).all() and (h[-PAD:] == 0xA5).all(), f"{name}: bytes outside the output were written"
    return q.cpu().numpy(), s.cpu().numpy(), z.cpu().numpy()


def assert_equal(got, want):
    (b, s, z), (eb, es, ez) = got, want
    np.testing.assert_array_equal(b.reshape(eb.shape), eb)
    assert s.tobytes() == es.tobytes()
    np.testing.assert_array_equal(z.reshape(-1), ez.reshape(-1))


def weight(k, n, seed=0):
    return np.random.default_rng(k * 131 + n + seed).standard_normal((k, n), dtype=np.float32)


@pytest.mark.parametrize("k,n", [(256, 128),      # one pair block, all eight waves
                                 (512, 132),      # a last column tile of 4 columns: three waves per k-group past N, one lane column live
                                 (384, 128),      # K / g = 3, odd: the four-wave build
                                 (1024, 644)],    # six column tiles x four row tiles: the chunked block order with a narrow last chunk
                         ids=["256x128", "512x132", "384x128-odd", "1024x644"])
def test_pair_blocks_vs_oracle(ops, k, n):
    w = weight(k, n)
    assert_equal(quantize_guarded(ops, dev(w), "uint4"), oracle(w, "uint4"))


def test_leading_dimension(ops):
    """A column slice of a wider matrix: ldw > N, 16-byte aligned start."""
    k, n = 256, 128
    wide = weight(k, n + 24)
    assert_equal(quantize_guarded(ops, dev(wide)[:, 8:8 + n], "uint4"), oracle(wide[:, 8:8 + n], "uint4"))


@pytest.mark.parametrize("qtype,sym", [("uint4", False), ("uint4", True), ("int4", False)], ids=["uint4", "uint4-symmetric", "int4"])
def test_grids(ops, qtype, sym):
    """int4 is the signed grid: the bias of the levels and the flipped nibbles."""
    w = weight(256, 128, 7)
    assert_equal(quantize_guarded(ops, dev(w), qtype, sym), oracle(w, qtype, sym))


def test_nonfinite_group_takes_the_fallback_from_lds(ops):
    """+inf and NaN in one (column, k-group): its range is NaN, the wave's rows are redone by the exact-division fallback, which reads
    the scales of all the wave's columns from LDS.  Every other (column, k-group) keeps the oracle's bits."""
    k, n = 256, 128
    w = weight(k, n, 3)
    w[130, 37] = np.inf
    w[200, 37] = np.nan
    (b, s, z), (eb, es, ez) = quantize_guarded(ops, dev(w), "uint4"), oracle(w, "uint4")
    ok = np.ones((n, k // G), bool)
    ok[37, 1] = False
    bad = ~np.isfinite(es.reshape(n, k // G))
    assert np.array_equal(bad, ~ok)
    assert np.array_equal(~np.isfinite(s.reshape(n, k // G)), bad)
    np.testing.assert_array_equal(b.reshape(eb.shape)[ok], eb[ok])
    assert s.reshape(n, k // G)[ok].tobytes() == es.reshape(n, k // G)[ok].tobytes()
    np.testing.assert_array_equal(z.reshape(n, k // G)[ok], ez.reshape(n, k // G)[ok])


def test_pointer_table_and_batch_equal_the_single_calls(ops):
    import torch
    k, n = 256, 128
    ws = [weight(k, n, 11), weight(k, n, 12)]
    single = [oracle(w, "uint4") for w in ws]
    for w, want in zip(ws, single):
        assert_equal(quantize_guarded(ops, dev(w), "uint4"), want)
    many = ops.rtn_quantize_many([dev(w) for w in ws], "uint4", G, layout="nbits")
    for (q, s, z), want in zip(many, single):
        assert_equal((q.cpu().numpy(), s.cpu().numpy(), z.cpu().numpy()), want)
    bq, bs, bz = ops.rtn_quantize_batched(torch.stack([dev(w) for w in ws]), "uint4", G, layout="nbits")
    for i, want in enumerate(single):
        assert_equal((bq[i].cpu().numpy(), bs[i].cpu().numpy(), bz[i].cpu().numpy()), want)
