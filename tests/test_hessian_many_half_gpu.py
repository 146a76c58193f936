"""The grouped GPTQ Hessian of fp16 / bf16 activations (csrc/syrk_bf16x3.hip section 4b, oq_hessian_accumulate_many_h16) and
what is built on it: the half partition of `ops.hessian_accumulate_many` and the calibration driver's grouped route.

Half x half products are exact in fp32, so integer data must come out bit for bit whatever the summation order; an item of up
to 992 rows runs the per-tensor call's single slice through the same device function and must give its bits; longer items are
held to the project's Hessian gate against float64 (1e-5 max |H|, tests/test_gptq_gpu.py).  The shapes are the smallest that
exercise the padding of both extents, the binary search over several items of different block counts, and both load paths
of the pack (dword loads, and 2-byte loads for an item on an odd leading dimension from an odd element offset)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ["float16", "bfloat16"]
GATE = 1e-5


@pytest.fixture(scope="module")
def ops():
    import torch
    from onnx_quantize_amd.hip import ops as _ops
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture
def restore_hessian_method(ops):
    before = ops.hessian_method()
    yield
    ops.hessian_set_method(before)


def tdtype(name):
    import torch
    return getattr(torch, name)


def many_h16(xs, hs, n_seen, n_add, dtype, *, workspace_bytes=None, xtype=None, ldx=None):
    """One oq_hessian_accumulate_many_h16 call on 2-D row-contiguous `xs`; returns (status, queried workspace bytes)."""
    import torch
    from onnx_quantize_amd.hip import _lib as L
    lib = L.load()
    rows = []
    for i, (x, h) in enumerate(zip(xs, hs)):
        assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == tdtype(dtype) and h.is_contiguous()
        rows.append((x.data_ptr(), h.data_ptr(), x.shape[0], x.shape[1], x.stride(0) if ldx is None or ldx[i] is None else ldx[i], n_seen[i],
                     n_add[i], 0))
    host = np.asarray(rows, dtype=np.int64)
    dev = torch.from_numpy(host).cuda()
    hp = C.c_void_p(host.ctypes.data)
    need = lib.oq_hessian_many_half_workspace_bytes(hp, len(rows))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
    st = lib.oq_hessian_accumulate_many_h16(hp, C.c_void_p(dev.data_ptr()), len(rows), L.WTYPE_CODE[dtype] if xtype is None else xtype,
                                            C.c_void_p(ws.data_ptr()), need if workspace_bytes is None else workspace_bytes,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, need


def h64(x, n_add):
    """(2 / n) X^T X of the exact values of a half tensor, in float64 on the device."""
    x64 = x.reshape(-1, x.shape[-1]).double()
    return (2.0 / n_add) * (x64.T @ x64)


def assert_within_gate(h, ref, what):
    top = float(ref.abs().max())
    ratio = float((h.double() - ref).abs().max()) / top
    print(f"{what}: max |H - H64| = {ratio:.3e} of max |H64|")
    assert ratio <= GATE, what


# ------------------------------------------------------------------------------------ 1. exact integers, through the C entry
def _integer_items(dtype):
    """(T 2048, K 640, n 4), (T 40, K 9, n 4), (T 33, K 257 on an odd ldx from an odd element offset, n 1), (T 512, K 520, n 2)."""
    import torch
    rng = np.random.default_rng(11)
    xs, want, n_add = [], [], [4, 4, 1, 2]
    for (t, k), n in zip([(2048, 640), (40, 9), (33, 257), (512, 520)], n_add):
        xi = rng.integers(-8, 9, size=(t, k))
        assert t * 64 < 2 ** 24                                           # every partial sum is an exact fp32 integer; 2 / n a power of two
        x = torch.from_numpy(xi.astype(np.float32)).cuda().to(tdtype(dtype))
        if (t, k) == (33, 257):
            ld = 259
            flat = torch.zeros(t * ld + 1, dtype=tdtype(dtype), device="cuda")
            view = flat[1:1 + t * ld].reshape(t, ld)[:, :k]
            view.copy_(x)
            assert view.data_ptr() % 4 == 2 and view.stride(0) % 2 == 1    # rows that are only 2-byte aligned
            x = view
        xs.append(x)
        want.append((xi.T @ xi).astype(np.float64) * (2.0 / n))
    return xs, want, n_add


@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_data_is_exact_for_every_item_of_a_mixed_table(dtype):
    import torch
    xs, want, n_add = _integer_items(dtype)
    hs = [torch.full((x.shape[1], x.shape[1]), 7.0, device="cuda") for x in xs]       # beta = 0: what H held is not read
    st, _ = many_h16(xs, hs, [0] * 4, n_add, dtype)
    assert st == 0
    for h, w in zip(hs, want):
        np.testing.assert_array_equal(h.cpu().numpy().astype(np.float64), w)
    for x, w, n in zip(xs, want, n_add):                                               # count = 1: a table of one item
        h = torch.full((x.shape[1], x.shape[1]), 7.0, device="cuda")
        assert many_h16([x], [h], [0], [n], dtype)[0] == 0
        np.testing.assert_array_equal(h.cpu().numpy().astype(np.float64), w)


# ------------------------------------------------------------------------------------ 2. the per-tensor call's bits up to 992 rows
@pytest.mark.parametrize("dtype", DTYPES)
def test_items_of_up_to_992_rows_get_the_bits_of_the_per_tensor_call(ops, dtype):
    import torch
    g = torch.Generator(device="cuda").manual_seed(2)
    xs = [torch.randn((4, t // 4, k), generator=g, device="cuda").to(tdtype(dtype)) for t, k in [(512, 1024), (992, 520), (768, 640)]]
    hs = [torch.zeros((x.shape[-1], x.shape[-1]), device="cuda") for x in xs]
    ref = [torch.zeros_like(h) for h in hs]
    for n_seen in ([0, 0, 0], [4, 12, 100]):
        flat = [x.reshape(-1, x.shape[-1]) for x in xs]
        assert many_h16(flat, hs, n_seen, [4, 4, 4], dtype)[0] == 0
        for x, r, n in zip(xs, ref, n_seen):
            assert ops.hessian_accumulate(x, r, n) == n + 4
        for i, (h, r) in enumerate(zip(hs, ref)):
            assert torch.equal(h, r), (i, n_seen)
    assert all(bool(h.abs().max() > 0) for h in hs)


# ------------------------------------------------------------------------------------ 3. long items against float64
@pytest.mark.parametrize("dtype", DTYPES)
def test_long_items_against_float64(dtype):
    import torch
    g = torch.Generator(device="cuda").manual_seed(3)
    xs = []
    for t, k in [(4096, 1024), (2050, 1301)]:
        x = torch.randn((t, k), generator=g, device="cuda") * (0.1 + 3 * torch.rand(k, generator=g, device="cuda")) + 0.25
        x[:, 5] = 0
        if dtype == "float16":
            x[:, 7] = torch.where(x[:, 7] < 0, -1.0, 1.0) * 2.0 ** -24               # fp16's smallest subnormal, either sign
        xs.append(x.to(tdtype(dtype)))
    hs = [torch.full((x.shape[1], x.shape[1]), 7.0, device="cuda") for x in xs]
    assert many_h16(xs, hs, [0, 0], [2, 2], dtype)[0] == 0
    for x, h in zip(xs, hs):
        assert_within_gate(h, h64(x, 2), f"{dtype} {tuple(x.shape)}")
        assert torch.equal(h, h.T)
        assert bool((h[5] == 0).all()) and bool((h[:, 5] == 0).all())
        if dtype == "float16":
            assert float(h[7, 7]) > 0


# ------------------------------------------------------------------------------------ 4. routing in ops
def test_ops_partitions_the_list_by_dtype_and_size(ops, monkeypatch, restore_hessian_method):
    import torch
    ops.hessian_set_method("auto")
    g = torch.Generator(device="cuda").manual_seed(4)
    rand = lambda shape, dt: torch.randn(shape, generator=g, device="cuda").to(dt)      # noqa: E731
    xs = [rand((2, 256, 512), torch.float32),                                          # fp32, eligible: the fp32 chain
          rand((2, 256, 520), torch.float16), rand((4, 160, 512), torch.float16),      # two fp16 eligible: one half chain
          rand((2, 256, 512), torch.bfloat16), rand((2, 300, 640), torch.bfloat16),    # two bf16 eligible: another
          rand((2, 128, 512), torch.float16)]                                          # 256 rows: per tensor
    hs = [torch.zeros((x.shape[-1], x.shape[-1]), device="cuda") for x in xs]
    calls = []
    real = ops.hessian_accumulate

    def recording(x, h, n_seen, method=None):
        calls.append(x)
        return real(x, h, n_seen, method)

    monkeypatch.setattr(ops, "hessian_accumulate", recording)
    assert ops.hessian_accumulate_many(xs, hs, [0] * 6) == [2, 2, 4, 2, 2, 2]
    assert len(calls) == 1 and calls[0] is xs[5]
    assert ops.hessian_accumulate_many(xs, hs, [2, 2, 4, 2, 2, 2]) == [4, 4, 8, 4, 4, 4]   # the running mean of the same X twice: the same H
    assert len(calls) == 2 and calls[1] is xs[5]
    monkeypatch.undo()
    torch.cuda.synchronize()
    for x, h in zip(xs, hs):
        assert_within_gate(h, h64(x, x.shape[0]), f"{x.dtype} {tuple(x.shape)}")
        assert torch.equal(h, h.T)
    # a single eligible half item: the per-tensor call, bit for bit
    for x in (xs[1], xs[4]):
        one, ref = (torch.zeros((x.shape[-1], x.shape[-1]), device="cuda") for _ in range(2))
        assert ops.hessian_accumulate_many([xs[0], x, xs[5]], [torch.zeros_like(hs[0]), one, torch.zeros_like(hs[5])], [0, 0, 0]) == [2, x.shape[0], 2]
        assert ops.hessian_accumulate(x, ref, 0) == x.shape[0]
        assert torch.equal(one, ref)


# ------------------------------------------------------------------------------------ 5. driver
def test_the_driver_groups_half_activations_without_an_fp32_copy(ops, monkeypatch, restore_hessian_method):
    import torch
    from onnx_quantize_amd.calibration_driver import ActivationStream
    g = torch.Generator(device="cuda").manual_seed(5)
    names = ["a", "b", "c"]
    batches = [{n: torch.randn((4, 128, 512), generator=g, device="cuda").half() for n in names} for _ in range(2)]
    refs = {n: h64(torch.cat([b[n] for b in batches]), 8) for n in names}
    half_types = (torch.float16, torch.bfloat16)
    upcasts = []                                                          # every half -> fp32 conversion while the stream is fed
    real_float, real_to = torch.Tensor.float, torch.Tensor.to

    def counting_float(self, *a, **kw):
        if self.dtype in half_types:
            upcasts.append("float")
        return real_float(self, *a, **kw)

    def counting_to(self, *a, **kw):
        if self.dtype in half_types and (torch.float32 in a or kw.get("dtype") is torch.float32):
            upcasts.append("to")
        return real_to(self, *a, **kw)

    for method in ("auto", "f32"):
        ops.hessian_set_method(method)
        many = {n: torch.zeros((512, 512), device="cuda") for n in names}
        seen = [0, 0, 0]
        for b in batches:
            seen = ops.hessian_accumulate_many([b[n] for n in names], [many[n] for n in names], seen)
        assert seen == [8, 8, 8]
        monkeypatch.setattr(torch.Tensor, "float", counting_float)
        monkeypatch.setattr(torch.Tensor, "to", counting_to)
        stream = ActivationStream(hessian_names=names)
        for b in batches:
            stream.feed({**b, "other": b["a"]})
        monkeypatch.undo()
        torch.cuda.synchronize()
        assert upcasts == [], method
        assert stream._side is None, method                               # no side streams: the grouped route
        assert sorted(stream.hessians) == names
        for n in names:
            acc = stream.hessians[n]
            assert acc.n == 8
            assert torch.equal(acc.h, many[n]), (method, n)
            assert_within_gate(acc.h, refs[n], f"driver, method {method}, tap {n}")


# ------------------------------------------------------------------------------------ 6. errors leave every H untouched
@pytest.mark.parametrize("dtype", DTYPES)
def test_library_errors_leave_every_h_untouched(dtype):
    import torch
    from onnx_quantize_amd.hip import _lib as L
    lib = L.load()
    xs = [torch.randn((t, k), device="cuda").to(tdtype(dtype)) for t, k in [(64, 40), (96, 300), (33, 17)]]
    hs = [torch.full((x.shape[1], x.shape[1]), 3.0, device="cuda") for x in xs]
    args = (xs, hs, [0, 0, 0], [1, 1, 1], dtype)
    st, need = many_h16(*args, workspace_bytes=1024)
    assert st == L.OQ_ERR_WORKSPACE and "workspace" in lib.oq_last_error().decode() and need > 1024
    st, _ = many_h16(*args, xtype=7)
    assert st == L.OQ_ERR_INVALID_ARGUMENT and "xtype" in lib.oq_last_error().decode()
    st, _ = many_h16(*args, ldx=[None, 299, None])
    assert st == L.OQ_ERR_INVALID_ARGUMENT and "item 1" in lib.oq_last_error().decode() and "ldx=299" in lib.oq_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((h == 3.0).all()) for h in hs)
    assert many_h16(*args)[0] == 0                                        # and the same call with what the query asks for runs
    for x, h in zip(xs, hs):
        assert not bool((h == 3.0).any())
        assert_within_gate(h, h64(x, 1), f"{dtype} {tuple(x.shape)}")
