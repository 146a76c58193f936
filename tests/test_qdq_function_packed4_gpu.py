"""`ops.qdq_function_packed4` / `oq_qdq_function_packed4` (include/oq_hip_qdq_function_packed4.h, csrc/qdq_function_packed4.hip): one
call of a QDQ function with quantized activations from a 4-bit weight as packed nibbles.  The reference is `qdq_function_cases.restate`
-- the header's arithmetic in NumPy, the integer product exact -- on the UNPACKED integers; every comparison is of bytes."""
import numpy as np
import pytest
import torch

from nbits_cases import plan
from qdq_function_cases import CHANNEL, COMBOS, INT4, MODE, TENSOR, UINT4, QCase, restate, same_bytes, where_wrong
from qlinear_cases import CODE

pytestmark = pytest.mark.gpu

# (M, K, N): the smallest call; K short of a 4-k run and N of a dword; exactly one of each; one past; one short of a step and of a
# column tile; exactly; one past; a second 128-row tile and three column tiles; split K with a short last split
SHAPES = [(1, 1, 2), (5, 3, 6), (16, 4, 8), (16, 5, 10), (33, 63, 126), (33, 64, 128), (33, 65, 130), (129, 200, 264), (16, 1088, 260)]
W_ZP = ["lo", "hi", None]       # along the table: the bottom / the top of the nibble range (per column: both, at the first and last), NULL


def pack(q):
    """[K, N] integers -> [K, N / 2] bytes as core/_pack.py orders them: the even column in the low nibble."""
    u = (q.to(torch.int16) & 15).to(torch.uint8)
    return u[:, 0::2] | (u[:, 1::2] << 4)


def case(seed, M, K, N, x_mode, out_mode, signed, w_zp="lo", w=None, **kw):
    """A QCase whose W and zero points lie in the 4-bit range of their 8-bit container, with its expected Y."""
    lo, dt = (-8, torch.int8) if signed else (0, torch.uint8)
    g = torch.Generator().manual_seed(seed)
    if w is None:
        w = torch.randint(lo, lo + 16, (K, N), generator=g).to(dt).cuda()
    c = QCase(seed, M, K, N, x_mode, out_mode, w_dt="i8" if signed else "u8", w=w, w_zp=None, **kw)
    if w_zp is not None:
        z = torch.randint(lo, lo + 16, (c.w_scale.numel(),), generator=g)
        z[0], z[-1] = (lo, lo + 15) if w_zp == "lo" else (lo + 15, lo)
        c.w_zp = z.to(dt).cuda()
        c.want = restate(*c._restate_args(out_mode, c.out_scale))[0]
    c.signed, c.packed = signed, pack(w)
    return c


def run(ops, c, packed=None):
    return ops.qdq_function_packed4(c.x, c.packed if packed is None else packed, c.w_scale, c.w_zp, n=c.N, signed=c.signed, **c.kwargs())


@pytest.fixture(scope="module")
def ops():
    from onnx_quantize_amd.hip import ops
    return ops


@pytest.mark.parametrize("signed", [True, False], ids=["int4", "uint4"])
@pytest.mark.parametrize("x_mode,out_mode", COMBOS)
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["x".join(map(str, s)) for s in SHAPES])
def test_every_mode_and_type_at_the_edges_of_the_staging_and_the_plan(ops, i, x_mode, out_mode, signed):
    M, K, N = SHAPES[i]
    if (M, K, N) == (16, 1088, 260):
        assert plan(M, K, N).splits > 1 and K % (plan(M, K, N).steps_per_split * 64) != 0
    c = case(100 + i, M, K, N, x_mode, out_mode, signed, w_zp=W_ZP[i % 3], gemm=i % 2 == 1, per_column=i % 4 < 2, x_dt=("u8", "i8")[i % 2],
             x_zp=None if i % 4 == 2 else ("mid", "lo", "hi")[i % 3])      # NULL goes with uint8: the type x is quantized to without one
    got = run(ops, c)
    assert same_bytes(got, c.want), where_wrong(got, c.want)


@pytest.mark.parametrize("signed", [True, False], ids=["int4", "uint4"])
@pytest.mark.parametrize("x_mode", ["static", "dynamic"])
def test_the_bytes_of_the_byte_route_on_the_unpacked_weight(ops, x_mode, signed):
    c = case(7, 33, 200, 130, x_mode, "static", signed, w_zp="hi", gemm=True)
    got, byte_route = run(ops, c), c.call(ops)
    assert torch.equal(got.view(torch.int32), byte_route.view(torch.int32)) and same_bytes(got, c.want), where_wrong(got, c.want)


@pytest.mark.parametrize("offset", range(4))
def test_rows_as_a_file_or_a_view_gives_them(ops, offset):
    """ldw > N / 2 with 0xFF in the gap (never read), a base at every offset mod 4 (byte loads), ldy > N with a sentinel (never written)."""
    from onnx_quantize_amd.hip import _lib as L
    M, K, N, ldw, ldy = 16, 77, 100, 57, 107
    c = case(11 + offset, M, K, N, "dynamic", None, offset % 2 == 0, w_zp="lo")
    buf = torch.full((offset + K * ldw,), 0xFF, dtype=torch.uint8, device="cuda")
    wv = buf[offset:].view(K, ldw)
    wv[:, :N // 2] = c.packed
    assert wv.data_ptr() % 4 == offset
    y = torch.full((M, ldy), -77.0, dtype=torch.float32, device="cuda")
    lib = L.load()
    need = lib.oq_qdq_function_packed4_workspace_bytes(M, K, N, MODE["dynamic"], MODE[None])
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = lib.oq_qdq_function_packed4(c.x.data_ptr(), 0, M, K, K, MODE["dynamic"], 0, None, None, wv.data_ptr(), INT4 if c.signed else UINT4, N, ldw,
                                     CHANNEL, 0, c.w_scale.data_ptr(), c.w_zp.data_ptr(), None, None, None, MODE[None], 0, None, None, y.data_ptr(),
                                     ldy, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0, lib.oq_last_error().decode()
    assert same_bytes(y[:, :N].contiguous(), c.want), where_wrong(y[:, :N].contiguous(), c.want)
    assert bool((y[:, N:] == -77.0).all())
    assert torch.equal(run(ops, c, wv).view(torch.int32), y[:, :N].contiguous().view(torch.int32))


def test_the_int32_sum_at_its_bound_and_the_refusal_one_past_it(ops):
    """K = 561433: S = 255 * 15 * K = 2147481225 < 2^31 (restate asserts it); K + 1 is refused before any launch."""
    from onnx_quantize_amd.hip import _lib as L
    K = ops.QDQ_FUNCTION_PACKED4_MAX_K
    assert K == 561433 and 255 * 15 * K == 2147481225 < 2 ** 31 <= 255 * 15 * (K + 1)
    w = torch.full((K + 1, 2), 15, dtype=torch.uint8, device="cuda")
    c = case(1, 1, K, 2, "static", None, False, w_zp=None, w=w[:K], x=np.full((1, K), 255.0, np.float32), x_scale=1.0, x_zp=None, w_scale=1.0,
             per_column=False)
    c.w_zp = torch.zeros(1, dtype=torch.uint8, device="cuda")
    assert int(c.S[0, 0]) == 2147481225
    got = run(ops, c)
    assert same_bytes(got, c.want), where_wrong(got, c.want)
    lib, x, y = L.load(), torch.full((1, K + 1), 255.0, device="cuda"), torch.full((1, 2), -77.0, device="cuda")
    assert lib.oq_qdq_function_packed4_workspace_bytes(1, K + 1, 2, MODE["static"], MODE[None]) == 0
    st = lib.oq_qdq_function_packed4(x.data_ptr(), 0, 1, K + 1, K + 1, MODE["static"], CODE[torch.uint8], c.x_scale.data_ptr(), None,
                                     pack(w).data_ptr(), UINT4, 2, 1, TENSOR, 0, c.w_scale.data_ptr(), c.w_zp.data_ptr(), None, None, None, MODE[None],
                                     0, None, None, y.data_ptr(), 2, None, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == L.OQ_ERR_UNSUPPORTED and "could wrap" in lib.oq_last_error().decode() and bool((y == -77.0).all())
    with pytest.raises(NotImplementedError, match="K = 561434"):
        ops.qdq_function_packed4(x, pack(w), c.w_scale, c.w_zp, n=2, signed=False, **c.kwargs())


@pytest.mark.parametrize("change,reason", [(dict(n=9), "an even N has a kernel"), (dict(w_scale=8), "grouped W"), (dict(x=torch.float16), "fp32 has a kernel"),
                                           (dict(w=torch.int8), "one value per byte keeps qdq_function")])
def test_the_refusals_by_name(ops, change, reason):
    c = case(3, 4, 64, 10, "static", None, True)
    x = c.x.to(change["x"]) if "x" in change else c.x
    w = torch.zeros((64, 10), dtype=torch.int8, device="cuda") if "w" in change else c.packed
    scale = torch.ones(change["w_scale"], device="cuda") if "w_scale" in change else c.w_scale
    with pytest.raises(NotImplementedError, match=reason):
        ops.qdq_function_packed4(x, w, scale, None, n=change.get("n", c.N), signed=True, **c.kwargs())
