"""Exact tests of the group-strategy RTN kernels (csrc/rtn.hip) where i.i.d. weights cannot reach: rounding boundaries, the block
order of the pair build, its parameter store arms and its right edges.  Everything -- integers, the bits of the scales, zero
points -- is compared with `oq_oracle` bit for bit, into buffers with 256 bytes of 0xA5 on either side that must survive.
tests/rtn_group_cases.py holds the inputs, the restated launch plans and the failure report; tests/test_rtn_group_cases.py shows
on the host that every case here is the test it claims to be."""
import ctypes as C

import numpy as np
import pytest

import rtn_group_cases as R

pytestmark = pytest.mark.gpu

PAD = 256


@pytest.fixture(scope="module")
def ops():
    import torch
    from onnx_quantize_amd.hip import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the shared inputs are read-only


class Guarded:
    """``nbytes`` of output that start ``lead`` bytes behind a 256-byte aligned address, PAD bytes of 0xA5 on either side."""

    def __init__(self, nbytes, lead=0):
        import torch
        self.lead, self.nbytes = lead, nbytes
        self.buf = torch.full((PAD + lead + nbytes + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.view = self.buf[PAD + lead:PAD + lead + nbytes]

    def check(self, what):
        h = self.buf.cpu().numpy()
        assert (h[:PAD + self.lead] == 0xA5).all() and (h[PAD + self.lead + self.nbytes:] == 0xA5).all(), f"{what}: bytes outside the output were written"

    def numpy(self, dtype=np.uint8):
        return self.view.cpu().numpy().view(dtype)


def q_bytes(k, n, g, bits, layout):
    return k * n if layout == "kn" else k * n * bits // 8


def outputs(ops, k, n, g, qtype, layout, batch=1, s_off=0, z_off=0, emit_q=True):
    import torch
    bits = 4 if "4" in qtype else 8
    count = n * k // g
    q = Guarded(batch * q_bytes(k, n, g, bits, layout)) if emit_q else None
    s, z = Guarded(batch * 4 * count, s_off), Guarded(batch * count, z_off)
    assert s.view.data_ptr() % 8 == s_off and z.view.data_ptr() % 2 == z_off % 2
    out = (None if q is None else q.view, s.view.view(torch.float32), z.view.view(ops.container_dtype(qtype)))
    return (q, s, z), out


def levels_of(q_guard, k, n, g, bits, layout, index=0):
    """The unsigned bytes / nibbles [K, N] of matrix ``index`` of a guarded integer output."""
    nb = q_bytes(k, n, g, bits, layout)
    raw = q_guard.numpy()[index * nb:(index + 1) * nb]
    if layout == "kn":
        return raw.reshape(k, n)
    if layout == "kn_packed4":
        return R.packed4_to_kn(raw, k, n)
    return R.blob_to_kn(raw, k, n, g, bits)


def assert_exact(guards, ref, k, n, g, bits, layout, lpr, index=0, what=""):
    """Matrix ``index`` of the guarded outputs against the oracle's (q, scale, zp), bit for bit."""
    qg, sg, zg = guards
    eq, es, ez = ref
    count = n * k // g
    if qg is not None:
        want = R.unsigned_levels(eq, 8 if layout == "kn" else bits)
        got = levels_of(qg, k, n, g, bits, layout, index)
        assert np.array_equal(got, want), what + " " + R.where_wrong(got, want, k, n, g, lpr)
    s = sg.numpy(np.float32)[index * count:(index + 1) * count]
    assert s.tobytes() == es.tobytes(), what + " " + R.where_params_wrong(s, es.reshape(-1), n, k // g, "scale")
    z = zg.numpy()[index * count:(index + 1) * count]
    ezb = ez.reshape(-1).view(np.uint8)
    assert np.array_equal(z, ezb), what + " " + R.where_params_wrong(z, ezb, n, k // g, "zero point")


def check_guards(guards):
    for name, gd in zip(("integers", "scale", "zero point"), guards):
        if gd is not None:
            gd.check(name)


def run_single(ops, w, ref, k, n, g, qtype, layout, lpr, sym=False, rr=False, clip=1.0, emit_q=True, s_off=0, z_off=0, what=""):
    bits = 4 if "4" in qtype else 8
    guards, out = outputs(ops, k, n, g, qtype, layout, 1, s_off, z_off, emit_q)
    q, _, _ = ops.rtn_quantize(dev(w), qtype, "group", g, sym, rr, clip, layout=layout, emit_q=emit_q, out=out)
    assert emit_q or q is None
    check_guards(guards)
    assert_exact(guards, ref, k, n, g, bits, layout, lpr, what=what)
    return guards


def announce(case):
    c = R.boundary_conditions(case.id)
    print(f"{case.id}: {case.k} x {case.n} g {case.g} {case.build}: naive_share {c['naive_share']:.4f}, fma form {c['fma_share']:.4f}, exact ties "
          f"{c['exact_ties']}, least used level {c['least_level'][0]} x {c['least_level'][1]}, strip rows {c['strip_rows']:.3f}")


# ------------------------------------------------------------------------------------ 1. boundary-dense inputs on every build
@pytest.mark.parametrize("case", R.BOUNDARY, ids=[c.id for c in R.BOUNDARY])
def test_boundary_dense_vs_oracle(ops, case):
    """Every element within two ulp of a rounding boundary of its own grid, none on an exact tie of the fast path's own arithmetic;
    one in thirty differs between rint(x * fl(1/s)) and the oracle, every row of every strip holds one: a band too narrow or from the
    wrong column, a fallback with another column's scale and a redo of the wrong row all change integers here."""
    announce(case)
    assert R.build_of(case.k, case.n, case.g, case.bits, case.layout, case.emit_q) == case.build
    w, ref = R.boundary_input(case.id)
    run_single(ops, w, ref, case.k, case.n, case.g, case.qtype, case.layout, case.lpr, case.symmetric, case.reduce_range, case.clip_ratio,
               case.emit_q, what=case.id)


@pytest.mark.parametrize("name,entry", R.LISTS, ids=[f"{a}-{b}" for a, b in R.LISTS])
def test_boundary_dense_through_the_list_and_the_batched_entry_points(ops, name, entry):
    import torch
    case = R.BOUNDARY_BY_ID[name]
    k, n, g = case.k, case.n, case.g
    inputs = [R.boundary_input(name), R.boundary_input(name, 1)]
    if entry == "many":
        got = ops.rtn_quantize_many([dev(w) for w, _ in inputs], case.qtype, g, layout=case.layout)
        assert len(got) == 2
        for i, ((q, s, z), (_, (eq, es, ez))) in enumerate(zip(got, inputs)):
            lv, want = R.blob_to_kn(q.cpu().numpy(), k, n, g, case.bits), R.unsigned_levels(eq, case.bits)
            assert np.array_equal(lv, want), f"matrix {i}: " + R.where_wrong(lv, want, k, n, g, case.lpr)
            assert s.cpu().numpy().tobytes() == es.tobytes(), f"matrix {i}: " + R.where_params_wrong(s.cpu().numpy(), es, n, k // g, "scale")
            assert np.array_equal(z.cpu().numpy().reshape(-1).view(np.uint8), ez.reshape(-1).view(np.uint8)), f"matrix {i}: zero points"
    else:
        guards, (q, s, z) = outputs(ops, k, n, g, case.qtype, case.layout, batch=2)
        count = n * k // g
        out = (q.view(2, n, k // g, g * case.bits // 8), s.view(2, count, 1), z.view(2, count, 1))
        ops.rtn_quantize_batched(torch.stack([dev(w) for w, _ in inputs]), case.qtype, g, layout=case.layout, out=out)
        check_guards(guards)
        for i, (_, ref) in enumerate(inputs):
            assert_exact(guards, ref, k, n, g, case.bits, case.layout, case.lpr, i, f"matrix {i}:")


# ------------------------------------------------------------------------------------ 2. block orders
@pytest.mark.parametrize("k,n,g,build,xg,arms,live", R.ORDERS, ids=[f"{o[0]}x{o[1]}-g{o[2]}" for o in R.ORDERS])
def test_block_orders_with_a_short_band_vs_oracle(ops, k, n, g, build, xg, arms, live):
    """`tile_of_block` order 2 under the pair build (row tiles halved, no k-group guard) and the five-wave g = 64 build: a full band
    followed by a short one, full chunks at xg_log2 0 .. 3, a narrow last chunk, a last tile of one live strip."""
    p = R.wave_plan(k, n, g, 4)
    assert (p["build"], p["xg_log2"], p["arms"], p["live_strips_of_last_tile"]) == (build, xg, arms, live)
    w, ref = R.normal_input(k, n, g)
    run_single(ops, w, ref, k, n, g, "uint4", "nbits", p["lpr"], what=f"{k} x {n}")


# ------------------------------------------------------------------------------------ 3. store arms of the pair build
@pytest.mark.parametrize("k,n", R.STORE_SHAPES, ids=[f"{k}x{n}" for k, n in R.STORE_SHAPES])
@pytest.mark.parametrize("s_off,z_off", R.STORE_OFFSETS, ids=[f"scale+{a}-zp+{b}" for a, b in R.STORE_OFFSETS])
def test_pair_parameter_stores_at_every_alignment(ops, k, n, s_off, z_off):
    """(s0, s1) leaves as one float2 or as two floats, the zero-point pair as one uint16_t or as two bytes, by the alignment of the
    caller's arrays: oq_hip.h promises 4-byte scales and zero points at any address."""
    assert R.wave_plan(k, n, 128, 4)["build"] == "pair"
    w, ref = R.normal_input(k, n, 128, seed=3)
    aligned = run_single(ops, w, ref, k, n, 128, "uint4", "nbits", 8)
    got = run_single(ops, w, ref, k, n, 128, "uint4", "nbits", 8, s_off=s_off, z_off=z_off, what=f"scale+{s_off} zp+{z_off}")
    for a, b in zip(aligned, got):
        assert a.numpy().tobytes() == b.numpy().tobytes()


@pytest.mark.parametrize("k,n", R.STORE_SHAPES, ids=[f"{k}x{n}" for k, n in R.STORE_SHAPES])
def test_pair_parameter_stores_through_a_pointer_table_of_mixed_alignments(ops, k, n):
    """oq_rtn_quantize_ptrs_f32 called directly: the alignment is decided per entry inside the kernel."""
    import torch
    from onnx_quantize_amd.hip import _lib as L
    lib = L.load()
    g, count = 128, len(R.TABLE_OFFSETS)
    inputs = [R.normal_input(k, n, g, seed=20 + i) for i in range(count)]
    wd = [dev(w) for w, _ in inputs]
    guards = [outputs(ops, k, n, g, "uint4", "nbits", 1, s_off, z_off)[0] for s_off, z_off in R.TABLE_OFFSETS]
    table = np.array([[wd[i].data_ptr(), gq.view.data_ptr(), gs.view.data_ptr(), gz.view.data_ptr()] for i, (gq, gs, gz) in enumerate(guards)],
                     dtype=np.int64)
    assert [int(t[2] % 8) for t in table] == [0, 4, 0] and [int(t[3] % 4) for t in table] == [0, 1, 3]
    table_dev = torch.from_numpy(table).cuda()
    wsb = torch.empty(max(int(lib.oq_rtn_batched_workspace_bytes(count, k, n, g)), 16), dtype=torch.uint8, device="cuda")
    L.check(lib.oq_rtn_quantize_ptrs_f32(C.c_void_p(table.ctypes.data), C.c_void_p(table_dev.data_ptr()), count, k, n, n, L.QTYPE_CODE["uint4"], g,
                                         0, 0, 1.0, L.OQ_LAYOUT_NBITS, C.c_void_p(wsb.data_ptr()), wsb.numel(),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for i, (gd, (w, ref)) in enumerate(zip(guards, inputs)):
        check_guards(gd)
        assert_exact(gd, ref, k, n, g, 4, "nbits", 8, what=f"entry {i} (scale+{R.TABLE_OFFSETS[i][0]}, zp+{R.TABLE_OFFSETS[i][1]}):")
        single = run_single(ops, w, ref, k, n, g, "uint4", "nbits", 8)
        for a, b in zip(single, gd):
            assert a.numpy().tobytes() == b.numpy().tobytes(), f"entry {i}"


@pytest.mark.parametrize("k,n", R.STORE_SHAPES, ids=[f"{k}x{n}" for k, n in R.STORE_SHAPES])
def test_pair_parameter_stores_of_a_batch_at_odd_addresses(ops, k, n):
    import torch
    g, count = 128, n * k // 128
    inputs = [R.normal_input(k, n, g, seed=20 + i) for i in range(3)]
    guards, (q, s, z) = outputs(ops, k, n, g, "uint4", "nbits", batch=3, s_off=4, z_off=1)
    out = (q.view(3, n, k // g, g // 2), s.view(3, count, 1), z.view(3, count, 1))
    ops.rtn_quantize_batched(torch.stack([dev(w) for w, _ in inputs]), "uint4", g, layout="nbits", out=out)
    check_guards(guards)
    for i, (_, ref) in enumerate(inputs):
        assert_exact(guards, ref, k, n, g, 4, "nbits", 8, i, f"matrix {i}:")


# ------------------------------------------------------------------------------------ 4. right edges of the pair build
@pytest.mark.parametrize("case", R.EDGES, ids=[c.id for c in R.EDGES])
def test_pair_right_edges_boundary_dense(ops, case):
    """A wave whose strip starts past N recomputes the block's first strip and leaves bytes nobody may store; with boundary-dense
    inputs those rows are redone too, and the guards and the neighbouring columns show any of them that is stored."""
    announce(case)
    p = R.wave_plan(case.k, case.n, case.g, 4)
    assert p["build"] == "pair"
    w, ref = R.boundary_input(case.id)
    run_single(ops, w, ref, case.k, case.n, case.g, case.qtype, "nbits", 8, what=case.id)
