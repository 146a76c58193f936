"""`ops.qdq_function_decode` / `oq_qdq_function_decode` (include/oq_hip_qdq_function_decode.h, csrc/qdq_function_decode.hip): the W8A8
QDQ function call for 1 ... 16 rows, the [K, N] bytes streamed once.  The reference is `qdq_function_cases.restate` -- the header's
arithmetic in NumPy, the integer product exact; every comparison is of bytes."""
import numpy as np
import pytest
import torch

from onnx_quantize_amd.hip import ops
from qdq_function_cases import CHANNEL, F16, F32, GROUP, MODE, TENSOR, UINT4, WTYPE, COMBOS, QCase, same_bytes, where_wrong
from qlinear_cases import CODE
from test_qdq_function_decode_abi import plan      # the header's plan, restated: (slice, splits)

pytestmark = pytest.mark.gpu


# (M, K, N).  M: one row, a partly filled A image, a full one.  K around a 16-k lane-group run and a 64-k span; N around a lane's 8
# bytes and the block (N = 128: the unguarded 8-byte loads).  Then two wide calls whose K splits with a short last slice: slice 128 on
# rows of 16385 bytes (byte loads), and slice 320 on 8-byte aligned rows (a wave's quarter of 80 is a whole span and a part of one).
SHAPES = [(1, 1, 1), (5, 15, 7), (16, 16, 8), (5, 17, 9), (1, 63, 127), (16, 64, 129), (5, 65, 128), (3, 330, 16385), (1, 1100, 16392)]


def run(c, w=None, fn="qdq_function_decode"):
    return getattr(ops, fn)(c.x, c.w if w is None else w, c.w_scale, c.w_zp, **c.kwargs())


def call_c(c, *, x=None, w=None, ldw=None, ldy=None, atype=F32, wtype=None, granularity=None):
    """`oq_qdq_function_decode` on QCase `c` into a Y of -77.0 with `ldy` columns: (status, its message, the workspace bytes, Y)."""
    from onnx_quantize_amd.hip import _lib as L
    lib = L.load()
    x, w = c.x if x is None else x, c.w if w is None else w
    M, K = x.shape
    ldw, ldy = c.N if ldw is None else ldw, c.N if ldy is None else ldy
    y = torch.full((M, ldy), -77.0, dtype=torch.float32, device="cuda")
    need = lib.oq_qdq_function_decode_workspace_bytes(M, K, c.N, MODE[c.x_mode], MODE[c.out_mode])
    ws = torch.empty(need, dtype=torch.uint8, device="cuda") if need else None
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    B, b_scale, b_zp = c.bias if c.bias is not None else (None, None, None)
    st = lib.oq_qdq_function_decode(x.data_ptr(), atype, M, K, K, MODE[c.x_mode], CODE[c.x_dt], ptr(c.x_scale), ptr(c.x_zp), w.data_ptr(),
                                    WTYPE[c.w_dt] if wtype is None else wtype, c.N, ldw,
                                    (CHANNEL if c.w_scale.numel() > 1 else TENSOR) if granularity is None else granularity, 0, ptr(c.w_scale),
                                    ptr(c.w_zp), ptr(B), ptr(b_scale), ptr(b_zp), MODE[c.out_mode], CODE[c.out_dt], ptr(c.out_scale), ptr(c.out_zp),
                                    y.data_ptr(), ldy, ptr(ws), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, lib.oq_last_error().decode(), need, y


@pytest.mark.parametrize("w_dt", ["u8", "i8"])
@pytest.mark.parametrize("x_mode,out_mode", COMBOS)
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["x".join(map(str, s)) for s in SHAPES])
def test_every_mode_and_type_at_the_edges_of_the_staging_and_the_plan(i, x_mode, out_mode, w_dt):
    M, K, N = SHAPES[i]
    assert plan(M, K, N) == {65: (64, 2), 330: (128, 3), 1100: (320, 4)}.get(K, (64, 1))      # a short last slice wherever K splits
    # i = 1, 5: "hi" per column (with uint8: zb' at both ends of its range); i = 3, 7: no w_zp (with int8: no row sums)
    c = QCase(400 + i, M, K, N, x_mode, out_mode, w_dt=w_dt, w_zp=("lo", "hi", "mid", None)[i % 4], gemm=i % 2 == 1, per_column=i % 3 != 0,
              x_dt=("u8", "i8")[i % 2], x_zp=None if i % 4 == 2 else ("mid", "lo", "hi")[i % 3])      # NULL goes with uint8: the type without one
    got = run(c)
    assert same_bytes(got, c.want), where_wrong(got, c.want)


@pytest.mark.parametrize("N,expected", [(1, (192, 173)), (1921, (2048, 17))])
def test_the_longest_k(N, expected):
    """K at its bound, 5 rows.  One column block: 173 slices, the last a single k.  16: slices of 2048, the cap (the LDS rows full), and one of 257."""
    K = ops.QDQ_FUNCTION_MAX_K
    assert plan(5, K, N) == expected and K % 192 == 1 and K % 2048 == 257
    c = QCase(5, 5, K, N, "static", None, w_dt="u8", w_zp="hi")
    got = run(c)
    assert same_bytes(got, c.want), where_wrong(got, c.want)


@pytest.mark.parametrize("x_mode,out_mode,gemm", [("static", "static", True), ("dynamic", "static", True), ("static", None, False), ("dynamic", "dynamic", False)])
def test_the_bytes_of_the_tile_route(x_mode, out_mode, gemm):
    c = QCase(7, 16, 200, 130, x_mode, out_mode, w_dt="i8" if gemm else "u8", w_zp="hi", gemm=gemm)
    got, tile = run(c), run(c, fn="qdq_function")
    assert torch.equal(got.view(torch.int32), tile.view(torch.int32)) and same_bytes(got, c.want), where_wrong(got, c.want)


@pytest.mark.parametrize("offset", range(4))
def test_rows_as_a_file_or_a_view_gives_them(offset):
    """ldw > N with 0xFF in the gap (never read), a base at offsets 0 ... 3 (beyond 0: byte loads), ldy > N with a sentinel (never written).
    The four kernels: odd offsets a static int8 X with a NULL zero point (no column sums), 2 and 3 an int8 W with one (no row sums)."""
    M, K, N, ldy = 16, 61, 100, 107
    ldw = 101 if offset else 104      # offset 0: 8-byte aligned rows, 8-byte loads next to the last lane's narrow ones
    x_mode = "static" if offset % 2 else "dynamic"
    c = QCase(11 + offset, M, K, N, x_mode, None, w_dt="i8" if offset >= 2 else "u8", w_zp=None if offset >= 2 else "hi", x_dt="i8", x_zp=None)
    buf = torch.full((offset + K * ldw,), 0xFF, dtype=torch.uint8, device="cuda")
    wv = buf[offset:].view(K, ldw).view(c.w.dtype)
    wv[:, :N] = c.w
    assert wv.data_ptr() % 8 == offset
    st, msg, need, y = call_c(c, w=wv, ldw=ldw, ldy=ldy)
    assert st == 0, msg
    assert (need == 0) == (x_mode == "static")      # one slice, nothing dynamic: no workspace, and NULL is taken
    assert same_bytes(y[:, :N].contiguous(), c.want), where_wrong(y[:, :N].contiguous(), c.want)
    assert bool((y[:, N:] == -77.0).all())


def test_the_int32_sum_at_its_bound():
    """K = 33025, every q_x and W 255 against zero points of 0: S = 255 * 255 * K = 2147450625 < 2^31 (restate asserts it)."""
    K = ops.QDQ_FUNCTION_MAX_K
    c = QCase(1, 1, K, 2, "static", None, w_dt="u8", w_zp=None, w=torch.full((K, 2), 255, dtype=torch.uint8, device="cuda"),
              x=np.full((1, K), 255.0, np.float32), x_scale=1.0, x_zp=None, w_scale=1.0, per_column=False)
    assert int(c.S[0, 0]) == 2147450625
    got = run(c)
    assert same_bytes(got, c.want), where_wrong(got, c.want)


@pytest.mark.parametrize("change,words,reason", [
    (dict(K=33026), "could wrap", "K = 33026"), (dict(M=17), "oq_qdq_function is the entry point", "17 rows .*qdq_function takes the rest"),
    (dict(atype=F16), "fp16 / bf16 X", "fp32 has a kernel"), (dict(granularity=GROUP), "grouped W", "grouped W"),
    (dict(wtype=UINT4), "oq_qdq_function_packed4_decode", None)])
def test_the_refusals_by_name_touch_nothing(change, words, reason):
    """Through the C entry point (Y keeps its sentinel) and through `ops`, for which a 4-bit code has no spelling."""
    from onnx_quantize_amd.hip import _lib as L
    c = QCase(3, 4, 64, 10, "static", None)
    M, K = change.get("M", 4), change.get("K", 64)
    x, w = torch.ones((M, K), device="cuda"), torch.ones((K, 10), dtype=torch.int8, device="cuda")
    st, msg, _, y = call_c(c, x=x, w=w, **{k: v for k, v in change.items() if k not in ("M", "K")})
    assert st == L.OQ_ERR_UNSUPPORTED and words in msg and bool((y == -77.0).all()), (st, msg)
    if reason:
        scale = torch.ones(8, device="cuda") if "granularity" in change else c.w_scale
        assert "17 rows" in ops.qdq_function_decode_unsupported(c.x, c.w, c.w_scale, c.w_zp, rows=17, **c.kwargs())      # `rows` overrides x's
        with pytest.raises(NotImplementedError, match=reason):
            ops.qdq_function_decode(x.half() if "atype" in change else x, w, scale, None, **c.kwargs())
