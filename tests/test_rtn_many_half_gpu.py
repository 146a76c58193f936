"""RTN on LISTS of fp16 / bf16 weights: oq_rtn_quantize_ptrs_h16 (csrc/rtn_half.hip, the fused half kernels with blockIdx.y =
entry of a device table of pointers) and `ops.rtn_quantize_model` on top of it.

The yardstick is `ops.rtn_quantize` on each tensor alone, which tests/test_rtn_half_gpu.py pins to the oracle and to the fp32
kernels: every (q, scale, zp) of a list call is `torch.equal` to it, scales compared as bytes.  One case per layout also goes
straight to the oracle on the upcast matrix.  The matrices come from `make_bits` of that file (zeros, constants, the type's
largest magnitudes next to subnormals and -0.0, exact rounding ties, group by group), a different seed per entry.

The shapes are the smallest at which the table kernels can go wrong: a sliver of one column tile, a ragged third block of
columns, every build of lane sets per group, the 32-row build, the thread-per-column kernel, and for the packed layout a number
of columns that is no multiple of 8 (byte stores, the last pair of columns in range)."""
import ctypes as C
import functools

import numpy as np
import pytest

import oq_oracle as O
from test_rtn_half_gpu import dev, make_bits, upcast

pytestmark = pytest.mark.gpu

WTYPES = ["float16", "bfloat16"]
WAVE_SHAPES = [(128, 8, 128), (256, 520, 128), (384, 1032, 16), (384, 1032, 32), (384, 1032, 64), (512, 16, 256)]
COLUMN_SHAPE = (96, 40, 48)
PACKED_ONLY_SHAPES = [(128, 36, 64), (128, 42, 64)]
TYPES = {"kn": [("uint4", False), ("int8", True)], "nbits": [("uint4", False), ("int8", True)], "kn_packed4": [("uint4", False), ("int4", True)]}


@pytest.fixture(scope="module")
def ops():
    import torch
    from onnx_quantize_amd.hip import ops as _ops
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(scope="module")
def lib():
    from onnx_quantize_amd.hip import _lib as L
    return L.load()


@functools.lru_cache(maxsize=None)
def bits_of(wtype, k, n, g, seed):
    """`make_bits`, made once per (type, shape, seed): the layouts of a shape share their matrices.  Nobody writes to the result."""
    return make_bits(wtype, k, n, g, seed)


def entries(wtype, k, n, g, count):
    """`count` separately allocated device matrices, a different seed per entry."""
    return [dev(bits_of(wtype, k, n, g, 1000 * e + k + n + g), wtype) for e in range(count)]


def same(got, ref):
    import torch
    (q, s, z), (rq, rs, rz) = got, ref
    assert q.dtype == rq.dtype and q.shape == rq.shape and z.dtype == rz.dtype and z.shape == rz.shape and s.shape == rs.shape
    assert s.dtype == torch.float32
    assert torch.equal(q, rq), "integers differ from the single call"
    assert torch.equal(z, rz), "zero points differ from the single call"
    assert s.cpu().numpy().tobytes() == rs.cpu().numpy().tobytes(), "scales differ from the single call"


def outputs(ops, k, n, g, qtype, layout, fill=None):
    """Separately allocated (q, scale, zp) of one matrix, shaped as `ops.rtn_quantize` returns them."""
    import torch
    q = ops._q_buffer(layout, (), k, n, g, qtype, "cuda")
    s = torch.empty((n * k // g, 1), dtype=torch.float32, device="cuda")
    z = torch.empty((n * k // g, 1), dtype=ops.container_dtype(qtype), device="cuda")
    if fill is not None:
        q.view(torch.uint8).fill_(fill)
        s.view(torch.uint8).fill_(fill)
        z.view(torch.uint8).fill_(fill)
    return q, s, z


def call_ptrs(ops, lib, ws, outs, qtype, g, sym, layout, null_device=False, edit=None):
    """oq_rtn_quantize_ptrs_h16 on the null stream; `edit(table)` may spoil the int64 [count, 4] table before it is uploaded."""
    import torch
    from onnx_quantize_amd.hip import _lib as L
    k, n = ws[0].shape
    table = np.array([[w.data_ptr(), q.data_ptr(), s.data_ptr(), z.data_ptr()] for w, (q, s, z) in zip(ws, outs)], dtype=np.int64)
    if edit is not None:
        edit(table)
    table_dev = torch.from_numpy(table).cuda()
    torch.cuda.synchronize()
    st = lib.oq_rtn_quantize_ptrs_h16(table.ctypes.data, None if null_device else table_dev.data_ptr(), len(ws), ops._HALF_WTYPE[ws[0].dtype], k, n,
                                      ws[0].stride(0), L.QTYPE_CODE[qtype], g, int(sym), 0, 1.0, ops._layout_code(layout), None)
    torch.cuda.synchronize()
    return st


# ------------------------------------------------------------------------------------ 1. per-entry bits
def shapes_of(layout):
    if layout == "kn_packed4":
        return WAVE_SHAPES + PACKED_ONLY_SHAPES
    return WAVE_SHAPES + [COLUMN_SHAPE]


CASES = [(layout, shape) for layout in TYPES for shape in shapes_of(layout)]


@pytest.mark.parametrize("wtype", WTYPES)
@pytest.mark.parametrize("layout,shape", CASES, ids=[f"{lay}-{'x'.join(map(str, s))}" for lay, s in CASES])
def test_every_entry_has_the_bits_of_the_single_call(ops, lib, wtype, layout, shape):
    k, n, g = shape
    ws = entries(wtype, k, n, g, 5)
    for qtype, sym in TYPES[layout]:
        ref = [ops.rtn_quantize(w, qtype, "group", g, sym, layout=layout) for w in ws]
        for count, null_device in ((1, True), (1, False), (2, False), (5, False)):
            outs = [outputs(ops, k, n, g, qtype, layout) for _ in range(count)]
            assert call_ptrs(ops, lib, ws[:count], outs, qtype, g, sym, layout, null_device) == 0, lib.oq_last_error()
            for got, r in zip(outs, ref):
                same(got, r)
        got = ops.rtn_quantize_model(ws, qtype, g, sym, layout=layout)
        assert len(got) == 5
        for one, r in zip(got, ref):
            same(one, r)


@pytest.mark.parametrize("wtype", WTYPES)
def test_the_column_kernel_refuses_the_packed_layout(ops, lib, wtype):
    import torch
    from onnx_quantize_amd.hip import _lib as L
    k, n, g = COLUMN_SHAPE
    ws = entries(wtype, k, n, g, 2)
    outs = [outputs(ops, k, n, g, "uint4", "kn_packed4", fill=0xA5) for _ in ws]
    assert call_ptrs(ops, lib, ws, outs, "uint4", g, False, "kn_packed4") == L.OQ_ERR_UNSUPPORTED
    assert b"KN_PACKED4" in lib.oq_last_error()
    for q, s, z in outs:
        assert all(bool((t.view(torch.uint8) == 0xA5).all()) for t in (q, s, z))
    # `rtn_quantize_model` serves it all the same: matrix by matrix through `rtn_quantize` (the [K, N] route and the packer)
    got = ops.rtn_quantize_model(ws, "uint4", g, layout="kn_packed4")
    for one, w in zip(got, ws):
        same(one, ops.rtn_quantize(w, "uint4", "group", g, layout="kn_packed4"))


@pytest.mark.parametrize("layout", ["kn", "nbits", "kn_packed4"])
def test_one_case_per_layout_against_the_oracle(ops, layout):
    import torch
    k, n, g, wtype = 256, 520, 128, "float16"
    seeds = [1000 * e + k + n + g for e in range(2)]
    got = ops.rtn_quantize_model(entries(wtype, k, n, g, 2), "uint4", g, layout=layout)
    for seed, (q, s, z) in zip(seeds, got):
        with np.errstate(all="ignore"):
            eq, es, ez = O.rtn_quantize(upcast(bits_of(wtype, k, n, g, seed), wtype), "uint4", "group", g, False, False, 1.0)
        assert s.cpu().numpy().tobytes() == np.asarray(es, np.float32).tobytes(), "scales differ from the oracle"
        np.testing.assert_array_equal(z.cpu().numpy(), ez)
        if layout == "kn":
            np.testing.assert_array_equal(q.cpu().numpy(), eq)
        elif layout == "nbits":
            blob, _, _ = O.matmul_nbits_layout(np.asarray(eq).astype(np.uint8), np.asarray(es), np.asarray(ez), g, 4)
            np.testing.assert_array_equal(q.cpu().numpy(), blob)
        else:
            packed = ops.pack_nibbles(torch.from_numpy(np.ascontiguousarray(eq).astype(np.uint8)).cuda())
            assert torch.equal(q.reshape(-1), packed)


# ------------------------------------------------------------------------------------ 2. a mixed list
def counted(monkeypatch, lib, name):
    """Wrap a bound C function: every call's (count, [W of each entry of the host table]) is recorded."""
    seen = []
    real = getattr(lib, name)

    def wrapper(table_host, table_device, count, *rest):
        addr = table_host.value if isinstance(table_host, C.c_void_p) else int(table_host)
        rows = np.ctypeslib.as_array((C.c_int64 * (4 * count)).from_address(addr)).reshape(count, 4)
        seen.append((count, [int(p) for p in rows[:, 0]]))
        return real(table_host, table_device, count, *rest)

    monkeypatch.setattr(lib, name, wrapper)
    return seen


@pytest.mark.parametrize("layout", ["kn", "nbits"])
def test_a_mixed_list_comes_back_in_input_order_one_call_per_group(ops, lib, monkeypatch, layout):
    import torch
    gs = 512                                               # clamped to K: g = K for the small matrices, 512 for the tall one
    assert ops.rtn_quantize_model([], "uint4", gs, layout=layout) == []
    f16 = lambda k, n, seed: dev(bits_of("float16", k, n, min(k, gs), seed), "float16")       # noqa: E731
    bf16 = lambda k, n, seed: dev(bits_of("bfloat16", k, n, min(k, gs), seed), "bfloat16")    # noqa: E731
    wide = dev(bits_of("float16", 128, 96, 128, 77), "float16")
    flat = torch.cat([torch.zeros(1, dtype=torch.float16, device="cuda"), f16(128, 72, 78).reshape(-1)])
    strided, odd, tall = wide[:, 8:80], flat[1:].view(128, 72), bf16(1024, 16, 79)
    assert strided.stride() == (96, 1) and odd.data_ptr() % 16 == 2 and odd.is_contiguous()
    ws = [f16(128, 72, 1).float(), f16(128, 72, 2), bf16(256, 40, 3), strided, f16(256, 40, 4).float(), bf16(128, 72, 5), f16(64, 24, 6),
          odd, f16(128, 72, 7), tall, bf16(256, 40, 8), f16(256, 40, 9), bf16(128, 72, 10).float(), bf16(128, 72, 11), f16(128, 72, 12)]
    ref = [ops.rtn_quantize(w, "uint4", "group", gs, layout=layout) for w in ws]
    half_calls = counted(monkeypatch, lib, "oq_rtn_quantize_ptrs_h16")
    f32_calls = counted(monkeypatch, lib, "oq_rtn_quantize_ptrs_f32")
    got = ops.rtn_quantize_model(ws, "uint4", gs, layout=layout)
    assert len(got) == len(ws)
    for one, r in zip(got, ref):
        same(one, r)
    # fp16 128x72 (3 aligned) | bf16 128x72 (2) | bf16 256x40 (2) | fp16 256x40 (1) | fp16 64x24 (1) | the strided view | the odd offset
    assert sorted(c for c, _ in half_calls) == [1, 1, 1, 1, 2, 2, 3]
    assert (1, [odd.data_ptr()]) in half_calls and (1, [strided.data_ptr()]) in half_calls
    grouped = {w.data_ptr() for w in ws if w.dtype != torch.float32 and w is not tall}
    assert {p for _, ptrs in half_calls for p in ptrs} == grouped                  # no fp32 item, not the g = 512 one
    assert sorted(c for c, _ in f32_calls) == [1, 2]                                # the fp32 items: `rtn_quantize_many`, by shape
    assert {p for _, ptrs in f32_calls for p in ptrs} == {w.data_ptr() for w in ws if w.dtype == torch.float32}


# ------------------------------------------------------------------------------------ 3. NaN containment across entries
@pytest.mark.parametrize("wtype", WTYPES)
@pytest.mark.parametrize("layout", ["kn", "kn_packed4"])
def test_a_nan_poisons_exactly_its_group_of_its_entry(ops, wtype, layout):
    import torch
    k, n, g, row, col = 256, 72, 128, 131, 17
    clean = [bits_of(wtype, k, n, g, 40 + e) for e in range(3)]
    dirty1 = clean[1].copy()
    dirty1[row, col] = 0x7E00 if wtype == "float16" else 0x7FC0
    a = ops.rtn_quantize_model([dev(b, wtype) for b in clean], "uint4", g, layout=layout)
    b = ops.rtn_quantize_model([dev(clean[0], wtype), dev(dirty1, wtype), dev(clean[2], wtype)], "uint4", g, layout=layout)
    for e in (0, 2):
        same(b[e], a[e])
    (q0, s0, z0), (q1, s1, z1) = a[1], b[1]
    s0, s1 = s0.cpu().numpy().reshape(-1), s1.cpu().numpy().reshape(-1)
    hit = col * (k // g) + row // g
    assert np.isnan(s1[hit]) and not np.isnan(s0[hit])
    keep = np.arange(s1.size) != hit
    assert s1[keep].tobytes() == s0[keep].tobytes(), "a neighbouring group's scale changed"
    assert np.array_equal(z1.cpu().numpy().reshape(-1)[keep], z0.cpu().numpy().reshape(-1)[keep])
    q0, q1 = q0.cpu().numpy(), q1.cpu().numpy()
    if layout == "kn_packed4":                              # [K, N/2]: two columns per byte, the even one in the low nibble
        q0 = np.stack([q0 & 0x0F, q0 >> 4], axis=-1).reshape(k, n)
        q1 = np.stack([q1 & 0x0F, q1 >> 4], axis=-1).reshape(k, n)
    same_q = np.ones((k, n), dtype=bool)
    same_q[row // g * g:row // g * g + g, col] = False
    assert np.array_equal(q1[same_q], q0[same_q])
    assert torch.equal(b[1][0], ops.rtn_quantize(dev(dirty1, wtype), "uint4", "group", g, layout=layout)[0])


# ------------------------------------------------------------------------------------ 4. no fp32 copy
def test_a_list_call_allocates_its_outputs_and_no_fp32_copy(ops):
    import torch
    g = torch.Generator(device="cuda").manual_seed(5)
    ws = [torch.randn((1024, 1024), generator=g, device="cuda").half() for _ in range(4)]
    res = ops.rtn_quantize_model(ws, "uint4", 128, layout="nbits")          # warm-up: the staging rows, the side stream
    del res
    ops.release_workspaces()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = ops.rtn_quantize_model(ws, "uint4", 128, layout="nbits")
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    out_bytes = sum(t.numel() * t.element_size() for r in res for t in r)
    assert out_bytes == 4 * (1024 * 1024 // 2 + 8192 * 4 + 8192)
    print(f"rise {rise} bytes, outputs {out_bytes} bytes")
    assert rise < out_bytes + (1 << 20), (rise, out_bytes)                    # an fp32 copy of ONE matrix is 4 MB


# ------------------------------------------------------------------------------------ 5. refusals leave everything untouched
def test_a_refused_table_names_the_entry_and_touches_no_output(ops, lib):
    import torch
    from onnx_quantize_amd.hip import _lib as L
    k, n, g = 128, 16, 128
    ws = entries("float16", k, n, g, 3)
    outs = [outputs(ops, k, n, g, "uint4", "kn", fill=0xA5) for _ in ws]

    def null_q_of_entry_2(table):
        table[2, 1] = 0

    def scale_of_entry_1_off_by_two(table):
        table[1, 2] += 2

    for edit, word in ((null_q_of_entry_2, b"entry 2"), (scale_of_entry_1_off_by_two, b"entry 1")):
        assert call_ptrs(ops, lib, ws, outs, "uint4", g, False, "kn", edit=edit) == L.OQ_ERR_INVALID_ARGUMENT
        assert word in lib.oq_last_error(), lib.oq_last_error()
        for q, s, z in outs:
            assert all(bool((t.view(torch.uint8) == 0xA5).all()) for t in (q, s, z)), "a refused call wrote an output"


# ------------------------------------------------------------------------------------ 6. sharding
def test_a_half_model_goes_through_the_sharded_entry_point(ops):
    """One process, no process group: the rank's share is the whole model."""
    import torch
    from onnx_quantize_amd import sharding as S
    shapes = [(512, 768), (256, 1024), (512, 768), (256, 1024), (512, 768)]
    specs = [S.LayerSpec(name=f"l{i}", k=k, n=n, tokens=0, hessian_key=f"l{i}") for i, (k, n) in enumerate(shapes)]
    g = torch.Generator(device="cuda").manual_seed(31)
    weights = {i: (torch.randn(kn, generator=g, device="cuda") * (0.5 + i)).half() for i, kn in enumerate(shapes)}
    out, _ = S.rtn_quantize_model_sharded(specs, weights, "uint4", 128, layout="nbits")
    assert list(out) == [sp.name for sp in specs]
    for i, sp in enumerate(specs):
        same(out[sp.name], ops.rtn_quantize(weights[i], "uint4", "group", 128, layout="nbits"))
