"""`ops.qdq_function_packed4_decode` / `oq_qdq_function_packed4_decode` (include/oq_hip_qdq_function_packed4_decode.h,
csrc/qdq_function_packed4_decode.hip): the W4A8 QDQ function call for 1 ... 16 rows, the packed nibbles streamed once.  The reference
is `qdq_function_cases.restate` -- the header's arithmetic in NumPy, the integer product exact -- on the UNPACKED integers; every
comparison is of bytes."""
import numpy as np
import pytest
import torch

from qdq_function_cases import CHANNEL, COMBOS, INT4, MODE, TENSOR, UINT4, same_bytes, where_wrong
from qlinear_cases import CODE
from test_qdq_function_packed4_gpu import W_ZP, case, pack

pytestmark = pytest.mark.gpu
BLOCK = 128      # a workgroup's columns: 16 column slots x one dword of 8 nibbles


def plan(M, K, N):
    """The header's plan: (slice, splits)."""
    want = -(-(512 if M <= 4 else 256) // -(-N // BLOCK))
    slice_ = min(2048, -(-(-(-K // want)) // 64) * 64)
    return slice_, -(-K // slice_)


# (M, K, N).  M: one row, a partly filled A image, a full one.  K around a 16-k lane-group run and a 64-k span (every slice here is 64,
# a wave's quarter 16: no whole span); N around a lane's dword and the block (N = 128: rows of 64 bytes, the unguarded dword loads).
# Then two wide calls whose K splits with a short last slice: slice 128 on rows of 8193 bytes (byte loads, a last block of 2
# columns), and slice 320 on 4-byte aligned rows (a wave's quarter of 80 is a whole span and a part of one: the pipeline).
SHAPES = [(1, 1, 2), (5, 15, 6), (16, 16, 8), (5, 17, 10), (1, 63, BLOCK - 2), (16, 64, BLOCK + 2), (5, 65, BLOCK), (3, 330, 16386), (1, 1100, 16392)]


def run(ops, c, packed=None, fn="qdq_function_packed4_decode"):
    return getattr(ops, fn)(c.x, c.packed if packed is None else packed, c.w_scale, c.w_zp, n=c.N, signed=c.signed, **c.kwargs())


@pytest.fixture(scope="module")
def ops():
    from onnx_quantize_amd.hip import ops
    return ops


@pytest.mark.parametrize("signed", [True, False], ids=["int4", "uint4"])
@pytest.mark.parametrize("x_mode,out_mode", COMBOS)
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["x".join(map(str, s)) for s in SHAPES])
def test_every_mode_and_type_at_the_edges_of_the_staging_and_the_plan(ops, i, x_mode, out_mode, signed):
    M, K, N = SHAPES[i]
    assert plan(M, K, N) == {65: (64, 2), 330: (128, 3), 1100: (320, 4)}.get(K, (64, 1))      # a short last slice wherever K splits
    c = case(300 + i, M, K, N, x_mode, out_mode, signed, w_zp=W_ZP[i % 3], gemm=i % 2 == 1, per_column=i % 4 < 2, x_dt=("u8", "i8")[i % 2],
             x_zp=None if i % 4 == 2 else ("mid", "lo", "hi")[i % 3])      # NULL goes with uint8: the type x is quantized to without one
    got = run(ops, c)
    assert same_bytes(got, c.want), where_wrong(got, c.want)


def test_the_longest_slice_fills_the_lds_rows(ops):
    """The longest K on one column block of more than 4 rows: slices of 2048, the cap, and a last one of 281."""
    M, K, N = 5, 561433, 2
    assert plan(M, K, N) == (2048, 275) and K % 2048 == 281
    c = case(5, M, K, N, "static", None, True, w_zp="hi")
    got = run(ops, c)
    assert same_bytes(got, c.want), where_wrong(got, c.want)


@pytest.mark.parametrize("x_mode,out_mode,gemm", [("static", "static", True), ("dynamic", "static", True), ("static", None, False), ("dynamic", "dynamic", False)])
def test_the_bytes_of_the_tile_route(ops, x_mode, out_mode, gemm):
    c = case(7, 16, 200, 130, x_mode, out_mode, signed=gemm, w_zp="hi", gemm=gemm)      # int4 with the Gemm, uint4 with the MatMul
    got, tile = run(ops, c), run(ops, c, fn="qdq_function_packed4")
    assert torch.equal(got.view(torch.int32), tile.view(torch.int32)) and same_bytes(got, c.want), where_wrong(got, c.want)


@pytest.mark.parametrize("offset", range(4))
def test_rows_as_a_file_or_a_view_gives_them(ops, offset):
    """ldw > N / 2 with 0xFF in the gap (never read), a base at every offset mod 4 (byte loads), ldy > N with a sentinel (never written).
    Odd offsets: a static int8 X with a NULL zero point, the call whose column sums are left out."""
    from onnx_quantize_amd.hip import _lib as L
    M, K, N, ldy = 16, 61, 100, 107
    ldw = 57 if offset else 60      # offset 0: aligned rows, dword loads next to the last block's narrow ones
    x_mode = "static" if offset % 2 else "dynamic"
    c = case(11 + offset, M, K, N, x_mode, None, offset < 2, w_zp="lo", x_dt="i8", x_zp=None)
    buf = torch.full((offset + K * ldw,), 0xFF, dtype=torch.uint8, device="cuda")
    wv = buf[offset:].view(K, ldw)
    wv[:, :N // 2] = c.packed
    assert wv.data_ptr() % 4 == offset
    y = torch.full((M, ldy), -77.0, dtype=torch.float32, device="cuda")
    lib = L.load()
    need = lib.oq_qdq_function_packed4_decode_workspace_bytes(M, K, N, MODE[x_mode], MODE[None])
    assert (need == 0) == (x_mode == "static")      # one slice, nothing dynamic: no workspace, and NULL is taken
    ws = torch.empty(need, dtype=torch.uint8, device="cuda") if need else None
    st = lib.oq_qdq_function_packed4_decode(c.x.data_ptr(), 0, M, K, K, MODE[x_mode], CODE[torch.int8], c.x_scale.data_ptr() if c.x_scale is not None else None,
                                            None, wv.data_ptr(), INT4 if c.signed else UINT4, N, ldw, CHANNEL, 0, c.w_scale.data_ptr(), c.w_zp.data_ptr(),
                                            None, None, None, MODE[None], 0, None, None, y.data_ptr(), ldy, ws.data_ptr() if need else None, need,
                                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0, lib.oq_last_error().decode()
    assert same_bytes(y[:, :N].contiguous(), c.want), where_wrong(y[:, :N].contiguous(), c.want)
    assert bool((y[:, N:] == -77.0).all())
    if x_mode == "dynamic":      # ops names the type of a static x by its zero point: int8 without one is the C entry point's alone
        assert torch.equal(run(ops, c, wv).view(torch.int32), y[:, :N].contiguous().view(torch.int32))


def test_the_int32_sum_at_its_bound_and_the_refusals_past_it_and_past_16_rows(ops):
    """K = 561433: S = 255 * 15 * K = 2147481225 < 2^31 (restate asserts it); K + 1 and M = 17 are refused before any launch."""
    from onnx_quantize_amd.hip import _lib as L
    K = ops.QDQ_FUNCTION_PACKED4_MAX_K
    w = torch.full((K + 1, 2), 15, dtype=torch.uint8, device="cuda")
    c = case(1, 1, K, 2, "static", None, False, w_zp=None, w=w[:K], x=np.full((1, K), 255.0, np.float32), x_scale=1.0, x_zp=None, w_scale=1.0,
             per_column=False)
    c.w_zp = torch.zeros(1, dtype=torch.uint8, device="cuda")
    assert int(c.S[0, 0]) == 2147481225
    got = run(ops, c)
    assert same_bytes(got, c.want), where_wrong(got, c.want)
    lib, stream = L.load(), torch.cuda.current_stream().cuda_stream
    for (M, Kx), status, words in (((1, K + 1), L.OQ_ERR_UNSUPPORTED, "could wrap"), ((17, 64), L.OQ_ERR_UNSUPPORTED, "oq_qdq_function_packed4 is the entry point")):
        x, y = torch.full((M, Kx), 255.0, device="cuda"), torch.full((M, 2), -77.0, device="cuda")
        assert lib.oq_qdq_function_packed4_decode_workspace_bytes(M, Kx, 2, MODE["static"], MODE[None]) == 0
        st = lib.oq_qdq_function_packed4_decode(x.data_ptr(), 0, M, Kx, Kx, MODE["static"], CODE[torch.uint8], c.x_scale.data_ptr(), None,
                                                pack(w).data_ptr(), UINT4, 2, 1, TENSOR, 0, c.w_scale.data_ptr(), c.w_zp.data_ptr(), None, None, None,
                                                MODE[None], 0, None, None, y.data_ptr(), 2, None, 0, stream)
        torch.cuda.synchronize()
        assert st == status and words in lib.oq_last_error().decode() and bool((y == -77.0).all())
    with pytest.raises(NotImplementedError, match="K = 561434"):
        ops.qdq_function_packed4_decode(torch.full((1, K + 1), 255.0, device="cuda"), pack(w), c.w_scale, c.w_zp, n=2, signed=False, **c.kwargs())
    with pytest.raises(NotImplementedError, match="17 rows .*qdq_function_packed4 takes the rest"):
        ops.qdq_function_packed4_decode(torch.zeros((17, K), device="cuda"), c.packed, c.w_scale, c.w_zp, n=2, signed=False, **c.kwargs())


@pytest.mark.parametrize("change,reason", [(dict(n=9), "an even N has a kernel"), (dict(w_scale=8), "grouped W"), (dict(x=torch.float16), "fp32 has a kernel"),
                                           (dict(w=torch.int8), "one value per byte keeps qdq_function")])
def test_the_refusals_by_name(ops, change, reason):
    c = case(3, 4, 64, 10, "static", None, True)
    x = c.x.to(change["x"]) if "x" in change else c.x
    w = torch.zeros((64, 10), dtype=torch.int8, device="cuda") if "w" in change else c.packed
    scale = torch.ones(change["w_scale"], device="cuda") if "w_scale" in change else c.w_scale
    with pytest.raises(NotImplementedError, match=reason):
        ops.qdq_function_packed4_decode(x, w, scale, None, n=change.get("n", c.N), signed=True, **c.kwargs())
