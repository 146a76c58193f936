"""HQQ straight from fp16 / bf16 weights (oq_hqq_optimize_h16, csrc/hqq.hip).

Both conversions to fp32 are exact and the arithmetic of HQQ stays fp32, so `hqq_quantize(w_half)` is DEFINED as
`hqq_quantize(w_half.float())`: the integers (both layouts), the scales, the float zero points and `rounds` are compared as raw
bytes (NaN patterns count) on every route -- the register-tile pass (groups of 16 .. 128 as fp32, 256 as packed halves), the
per-round route, views with a leading dimension and rows that are only 2-byte aligned.  One case goes straight against the
oracle with the tolerances tests/test_hqq.py states."""
import ctypes as C

import numpy as np
import pytest

import oq_oracle as O
from hqq_cases import integers_given

pytestmark = pytest.mark.gpu

DTYPES = ["float16", "bfloat16"]
GROUPS = [16, 32, 64, 128, 256]
ARGUMENTS = (dict(), dict(early_stop=False, iters=9), dict(kappa=3.0, iters=12), dict(iters=1), dict(reduce_range=True),
             dict(kappa=3.0, iters=32))      # the last one: the error rises after 13 to 19 rounds (the oracle's trace): a real early stop


def _same(a, b):
    """q, scale, zero point and rounds of two `hqq_quantize` results, bit for bit."""
    import torch
    if (a[0] is None) != (b[0] is None) or int(a[3]) != int(b[3]):
        return False
    if a[0] is not None and not (a[0].dtype == b[0].dtype == torch.uint8 and a[0].shape == b[0].shape and torch.equal(a[0], b[0])):
        return False
    return all(x.dtype == y.dtype == torch.float32 and x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))
               for x, y in ((a[1], b[1]), (a[2], b[2])))


_BASES = {}


def _bases(dtype):
    """The base matrices of one element type, made once: 512 x 600 and a 601-wide one for rows that are only 2-byte aligned."""
    import torch
    if dtype not in _BASES:
        gen = torch.Generator(device="cuda").manual_seed(160 + len(dtype))
        dt = getattr(torch, dtype)
        big = (torch.randn((512, 600), generator=gen, device="cuda") * (0.5 + torch.rand(600, generator=gen, device="cuda"))).to(dt)
        odd = (torch.randn((512, 601), generator=gen, device="cuda") * (0.5 + torch.rand(601, generator=gen, device="cuda"))).to(dt)
        _BASES[dtype] = (big, odd)
    return _BASES[dtype]


@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_half_weights_give_the_fp32_route_s_bits(dtype, g):
    import torch
    from onnx_quantize_amd.hip import ops
    big, odd = _bases(dtype)
    unaligned = odd[2:258, 3:136]                         # ldw 601, first element 1205: every other row starts on an odd element
    assert unaligned.data_ptr() % 4 == 2 and unaligned.stride(0) % 2 == 1
    views = (big[:, :520], big[:256, 8:140], unaligned, big[:g, :520])          # ldw 600; ragged columns; K = g: a single group
    for i, w in enumerate(views):
        assert w.dtype == getattr(torch, dtype) and not w.is_contiguous()
        w32 = w.float()
        for kwargs in (ARGUMENTS if i == 0 else (dict(), dict(kappa=3.0, iters=12))):
            got = ops.hqq_quantize(w, g, **kwargs)
            per_round = ops.hqq_quantize(w, g, per_round_launches=True, **kwargs)
            assert _same(got, ops.hqq_quantize(w32, g, **kwargs)), (dtype, g, i, kwargs)
            assert _same(got, per_round), (dtype, g, i, kwargs)                  # the one-pass route, g = 256 included
            assert _same(per_round, ops.hqq_quantize(w32, g, per_round_launches=True, **kwargs)), (dtype, g, i, kwargs)
            assert 1 <= int(got[3]) <= kwargs.get("iters", 20)
        for kwargs in (dict(layout="nbits"), dict(layout="nbits", per_round_launches=True), dict(emit_q=False)):
            assert _same(ops.hqq_quantize(w, g, **kwargs), ops.hqq_quantize(w32, g, **kwargs)), (dtype, g, i, kwargs)
    stopped = ops.hqq_quantize(views[0], g, kappa=3.0, iters=32)
    assert 1 < int(stopped[3]) < 32, int(stopped[3])                              # the early stop really triggers
    # more rounds than the one-pass kernel holds: the per-round route by itself
    w = views[0]
    long = ops.hqq_quantize(w, g, iters=40, early_stop=False)
    assert int(long[3]) == 40 and _same(long, ops.hqq_quantize(w.float(), g, iters=40, early_stop=False))


SPECIALS = {"float16": (65504.0, -65504.0, 2.0 ** -24, 0.0, -0.0), "bfloat16": (3.39e38, -3.39e38, 2.0 ** -133, 0.0, -0.0)}


@pytest.mark.parametrize("g", [64, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values_and_nan(dtype, g):
    """The largest finite values, a subnormal and both zeros in the first, a middle and the last row of a group; then a NaN,
    which poisons its own group (and, through the one global error, the decisions) but no other group's scale."""
    import torch
    from onnx_quantize_amd.hip import ops
    dt = getattr(torch, dtype)
    clean = _bases(dtype)[0][:, :300].clone()
    w = clean.clone()
    col = 0
    for row in (0, g // 2 - 1, g - 1):                   # of group 0, and the same rows of the last group
        for value in SPECIALS[dtype]:
            w[row, col] = value
            w[512 - g + row, col + 150] = value
            col += 1
    assert torch.isfinite(w.float()).all() and (w.float() != 0).sum() < w.numel()
    sub = torch.tensor(SPECIALS[dtype][2], dtype=dt)
    assert float(sub) == SPECIALS[dtype][2] and 0 < float(sub) < float(torch.finfo(dt).tiny)        # a subnormal of the type
    for kwargs in (dict(), dict(per_round_launches=True), dict(layout="nbits")):
        assert _same(ops.hqq_quantize(w, g, **kwargs), ops.hqq_quantize(w.float(), g, **kwargs)), (dtype, g, kwargs)
    poisoned = clean.clone()
    poisoned[g + 3, 7] = float("nan")                    # group 1 of column 7
    for kwargs in (dict(), dict(per_round_launches=True)):
        got = ops.hqq_quantize(poisoned, g, **kwargs)
        assert _same(got, ops.hqq_quantize(poisoned.float(), g, **kwargs)), (dtype, g, kwargs)
        s = got[1].reshape(300, 512 // g)
        s_clean = ops.hqq_quantize(clean, g, **kwargs)[1].reshape(300, 512 // g)
        keep = torch.ones_like(s, dtype=torch.bool)
        keep[7, 1] = False
        assert torch.equal(s[keep].view(torch.int32), s_clean[keep].view(torch.int32))
        assert torch.isnan(got[2].reshape(300, 512 // g)[7, 1]) or torch.isnan(s[7, 1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_half_weights_against_the_oracle(dtype):
    """256 x 192, g = 64, the oracle on the upcast matrix: the tolerances tests/test_hqq.py states and measured."""
    import torch
    from onnx_quantize_amd.hip import ops
    w16 = torch.from_numpy(np.random.default_rng(5).standard_normal((256, 192), dtype=np.float32)).cuda().to(getattr(torch, dtype))
    w = w16.float().cpu().numpy()
    q, s, z, rounds = ops.hqq_quantize(w16, 64)
    eq, es, ez = O.hqq_quantize(w, 64)
    q, s, z = q.cpu().numpy(), s.cpu().numpy(), z.cpu().numpy()
    assert s.tobytes() == es.tobytes()
    assert z.shape == ez.shape and z.dtype == np.float32
    assert q.tobytes() == integers_given(w, s, z, 64).tobytes()        # exact given the zero points the kernel returned
    assert np.abs(z - ez).max() <= 2e-5
    diff = q.astype(np.int16) - eq.astype(np.int16)
    assert np.abs(diff).max() <= 1
    assert np.count_nonzero(diff) / diff.size <= 1e-3
    rows = O.to_rows(w, "group", 64)
    s0, z0 = O.qparams_from_rows(rows, "uint4", "group", False, False, 1.0, False, np.float32, np.float32)
    trace = []
    O.hqq_optimize_zero_point(rows, s0, z0, False, 0.7, 10.0, 1.01, 20, True, trace=trace)
    assert int(rounds.item()) == len(trace)


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_fp32_copy_of_the_weight_is_made(dtype):
    """The rise of the allocated bytes during a call covers q (a byte per element) and the parameters (about 0.1 byte per
    element); the workspace is kept from the warm call.  An fp32 copy alone would be four bytes per element."""
    import torch
    from onnx_quantize_amd.hip import ops
    w = (torch.randn((2048, 2048), device="cuda") * 0.1).to(getattr(torch, dtype))
    out = ops.hqq_quantize(w, 128)
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = ops.hqq_quantize(w, 128)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert out[0].shape == (2048, 2048)
    assert rise < 2 * w.numel(), (rise, w.numel())


# ------------------------------------------------------------------------------------ seam and mirror
class _Tensor:
    def __init__(self, a):
        self._a = a

    def numpy(self):
        return self._a


class _Value:
    def __init__(self, name, const_value=None):
        self.name, self.const_value = name, const_value


@pytest.mark.parametrize("g", [32, 256])
@pytest.mark.parametrize("flagged", [False, True], ids=["plain", "matmul_nbits"])
def test_seam_takes_half_weights_for_hqq(flagged, g):
    """The three arrays for an np.float16 value and for resident fp16 / bf16 values: the bytes of the fp32 twin."""
    import torch
    from onnx_quantize_amd import HqqConfig, QConfig, QuantType, QWeightArgs, seam
    w16 = np.random.default_rng(31).standard_normal((512, 64)).astype(np.float16)
    qc = QConfig(weights=QWeightArgs(dtype=QuantType.from_string("uint4"), group_size=g, strategy="group", algorithm=HqqConfig(iters=10)))
    run = lambda value: seam.weight_arrays(value, qc, None, flagged)      # noqa: E731
    ref = run(_Value("fc.weight", _Tensor(w16.astype(np.float32))))
    got = run(_Value("fc.weight", _Tensor(w16)))
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    for dt in (torch.float16, torch.bfloat16):
        resident = torch.from_numpy(w16).cuda().to(dt)
        value = _Value("fc.weight", _Tensor(np.zeros((512, 64), np.float16)))
        value.device_value, value.placeholder = resident, True
        got = run(value)
        ref = run(_Value("fc.weight", _Tensor(resident.float().cpu().numpy())))
        for a, b in zip(got, ref):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_functional_mirror_uploads_float16_as_it_is(monkeypatch):
    import onnx_quantize_amd.staging as staging
    from onnx_quantize_amd import QuantType
    from onnx_quantize_amd.algorithms import _hqq_quantize
    seen = []
    real = staging.upload

    def spy(a, keep_half=False):
        t = real(a, keep_half=keep_half)
        seen.append((a.dtype, keep_half, t.dtype))
        return t

    monkeypatch.setattr(staging, "upload", spy)
    import torch
    w16 = np.random.default_rng(77).standard_normal((256, 96)).astype(np.float16)
    for g in (64, 256):
        got = _hqq_quantize(w16, QuantType.QUInt4, g)
        ref = _hqq_quantize(w16.astype(np.float32), QuantType.QUInt4, g)
        for a, b in zip(got, ref):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert seen[0] == (np.dtype(np.float16), True, torch.float16) and seen[1] == (np.dtype(np.float32), True, torch.float32)
    assert all(keep for _, keep, _ in seen) and len(seen) == 4


# ------------------------------------------------------------------------------------ refusals
def test_refusals():
    import torch
    from onnx_quantize_amd.hip import _lib as L
    from onnx_quantize_amd.hip import ops
    with pytest.raises(TypeError):
        ops.hqq_quantize(torch.zeros((64, 64), dtype=torch.float16), 32)         # a CPU tensor: no fallback
    with pytest.raises(TypeError):
        ops.hqq_quantize(torch.zeros((64, 64), dtype=torch.float64, device="cuda"), 32)
    # groups that straddle columns, through the raw call: the library's own status, nothing written
    lib = L.load()
    k, n, g = 96, 64, 64
    w = torch.randn((k, n), device="cuda").to(torch.bfloat16)
    scale = torch.ones(k * n // g, device="cuda")
    zp_in = torch.full((k * n // g,), 7.0, device="cuda")
    q = torch.full((k, n), 0xAB, dtype=torch.uint8, device="cuda")
    zp = torch.full((k * n // g,), -3.0, device="cuda")
    rounds = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    st = lib.oq_hqq_optimize_h16(C.c_void_p(w.data_ptr()), L.OQ_W_BF16, k, n, n, g, 0, C.c_void_p(scale.data_ptr()), C.c_void_p(zp_in.data_ptr()),
                                 0.7, 10.0, 1.01, 20, 1, 0, C.c_void_p(q.data_ptr()), L.OQ_LAYOUT_KN, C.c_void_p(zp.data_ptr()),
                                 C.c_void_p(rounds.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == L.OQ_ERR_UNSUPPORTED and "straddle" in lib.oq_last_error().decode()
    torch.cuda.synchronize()
    assert bool((q == 0xAB).all()) and bool((zp == -3.0).all()) and int(rounds) == 77 and not bool(ws.any())
    with pytest.raises(L.OqHipError) as e:
        ops.hqq_quantize(w, g)
    assert e.value.status == L.OQ_ERR_UNSUPPORTED
