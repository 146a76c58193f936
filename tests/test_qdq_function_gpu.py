"""`ops.qdq_function` / `oq_qdq_function` (include/oq_hip_qdq_function.h, csrc/qdq_function.hip): one call of a `quant`-domain QDQ
function with quantized activations, fp32 X in and fp32 Y out, the product on the int8 matrix cores.

Every comparison is of BYTES against `qdq_function_cases.restate`: the header's arithmetic block in NumPy, np.float32 operation by
operation in the stated order, the integer product exact.

1  the six mode combinations x MatMul / Gemm over the (M, K, N) table of test_qlinear_matmul_gpu.py; signs and zero-point forms.
2  the identity probe W = I_K.
3  gaps, alignments, a 512-tile grid four times over.
4  the dynamic parameters of the input and of the output at their edges; the static output's ties and saturation.
5  the bound against real arithmetic; peak memory.
"""
import numpy as np
import pytest
import torch

from nbits_cases import plan
from qdq_function_cases import COMBOS, DYNAMIC, MODE, QCase, dyn_params, raw, same_bytes, where_wrong, workspace
from qlinear_cases import RANGE, SIGNS
from qlinear_function_cases import F
from test_qlinear_matmul_gpu import SWEEP

pytestmark = pytest.mark.gpu

DT = {"u8": torch.uint8, "i8": torch.int8}
ZP_OF = {"lo": ("lo", "lo"), "hi": ("hi", "hi"), "mid": ("mid", "mid"), "null": (None, None), "a_null": (None, "lo"), "b_null": ("lo", None)}


@pytest.fixture(scope="module")
def ops():
    from onnx_quantize_amd.hip import ops
    return ops


@pytest.fixture(scope="module")
def lib():
    from onnx_quantize_amd.hip import _lib
    return _lib.load()


def combo_id(c):
    return f"{c[0]}-{c[1] or 'none'}"


# ------------------------------------------------------------------------------------ 1. modes, table, signs, zero points
@pytest.mark.parametrize("gemm", [False, True], ids=["MatMul", "Gemm"])
@pytest.mark.parametrize("combo", COMBOS, ids=combo_id)
def test_every_mode_over_the_table(lib, combo, gemm):
    """The table of the integer kernel (partial tiles; K one short of and one past a step; split K with a short last split) with its
    zero-point forms; the signs, per-tensor / per-column W parameters and the output type alternate along the table."""
    bad = []
    for i, (M, K, N, zp, why) in enumerate(SWEEP):
        xs, ws = SIGNS[i % 4]
        c = QCase(400 + i, M, K, N, combo[0], combo[1], x_dt=xs, w_dt=ws, x_zp=ZP_OF[zp][0], w_zp=ZP_OF[zp][1], out_zp=("lo", "hi", None)[i % 3],
                  out_dt=("u8", "i8")[i % 2], gemm=gemm, per_column=i % 3 != 0, b_zp=i % 2 == 0)
        st, y = raw(lib, c)
        assert st == 0, lib.oq_last_error().decode()
        if not same_bytes(y, c.want):
            bad.append(f"{(M, K, N, zp)} [{why}]: {where_wrong(y, c.want)}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("out_mode", [None, "static", "dynamic"], ids=["none", "static", "dynamic"])
@pytest.mark.parametrize("signs", SIGNS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_static_input_with_every_sign_and_zero_point_form(lib, signs, out_mode):
    """Through the C ABI: a NULL zero point of a signed type has no spelling in `ops.qdq_function`, which reads the type from it."""
    for x_zp, w_zp, out_zp in (("lo", "lo", "lo"), ("hi", "hi", "hi"), (None, None, None), ("mid", "lo", "mid")):
        for per_column in (False, True):
            c = QCase(17, 33, 200, 130, "static", out_mode, x_dt=signs[0], w_dt=signs[1], x_zp=x_zp, w_zp=w_zp, out_zp=out_zp, out_dt=signs[1],
                      gemm=per_column, per_column=per_column)
            st, y = raw(lib, c)
            assert st == 0 and same_bytes(y, c.want), (x_zp, w_zp, out_zp, per_column, where_wrong(y, c.want))


@pytest.mark.parametrize("out_mode", [None, "static", "dynamic"], ids=["none", "static", "dynamic"])
@pytest.mark.parametrize("w_dt", ["u8", "i8"])
def test_dynamic_input_with_both_weight_types(ops, w_dt, out_mode):
    for w_zp in ("lo", "hi", None):
        for per_column in (False, True):
            c = QCase(19, 33, 200, 130, "dynamic", out_mode, w_dt=w_dt, w_zp=w_zp, gemm=not per_column, per_column=per_column)
            y = c.call(ops)
            assert same_bytes(y, c.want), (w_zp, per_column, where_wrong(y, c.want))


# ------------------------------------------------------------------------------------ 2. the identity probe
@pytest.mark.parametrize("x_mode", ["static-u8", "static-i8", "dynamic"])
def test_the_identity_probe_shows_the_quantized_bytes(ops, x_mode):
    """W = I_K (int8, no zero point), w_scale = 1, no output Q -> DQ: Y = (q_x - zp_x) * x_scale.  With the static scale 2^-5 that is
    exact, so Y / s + zp IS q_x; the dynamic input is compared with the restatement."""
    rng = np.random.default_rng(5)
    for K in (1, 15, 16, 17, 64, 65):
        eye = torch.eye(K, dtype=torch.int8, device="cuda")
        x = (rng.standard_normal((16, K)) * 3).astype(F)
        if x_mode == "dynamic":
            c = QCase(5, 16, K, K, "dynamic", None, w=eye, w_zp=None, per_column=False, w_scale=1.0, x=x)
            assert same_bytes(c.call(ops), c.want), (K, where_wrong(c.call(ops), c.want))
            continue
        dt = x_mode[-2:]
        c = QCase(5, 16, K, K, "static", None, x_dt=dt, x_zp="mid", w=eye, w_zp=None, per_column=False, w_scale=1.0, x=x, x_scale=2.0 ** -5)
        y = c.call(ops).cpu().numpy()
        assert same_bytes(y, c.want)
        zp = int(c.x_zp)
        q = y / F(2.0 ** -5) + F(zp)
        lo, hi = RANGE[DT[dt]]
        want_q = np.clip(np.rint(x / F(2.0 ** -5)) + F(zp), lo, hi)
        assert np.array_equal(q, want_q), (K, np.argwhere(q != want_q)[:4])


# ------------------------------------------------------------------------------------ 3. gaps, alignments, a large grid
@pytest.mark.parametrize("combo", [("static", "static"), ("dynamic", "dynamic")], ids=combo_id)
def test_gaps_odd_bases_and_strided_views_give_the_contiguous_bytes(lib, combo):
    """lda > K with NaN and 3e38 in the gap (never read -- the min / max pass included), X offset by one float (rows 4-byte aligned
    only), every alignment of W mod 4 with a sentinel in its gap, ldy > N with a sentinel in the gap (never written)."""
    M, K, N = 16, 77, 100
    c = QCase(21, M, K, N, combo[0], combo[1], gemm=True)
    for (lda, offset), w_off in zip(((K + 2, 0), (K + 2, 1), (80, 0), (K, 1)), (0, 1, 2, 3)):
        buf = torch.full((M * lda + 4,), float("nan"), dtype=torch.float32, device="cuda")
        buf[1::2] = 3e38
        x = buf[offset: offset + M * lda].view(M, lda)[:, :K]
        x.copy_(c.x)
        assert x.data_ptr() % 16 == (4 * offset) % 16
        ldw = N + 3
        w_buf = torch.full((K * ldw + 4,), 0x55, dtype=c.w.dtype, device="cuda")
        w = w_buf[w_off: w_off + K * ldw].view(K, ldw)[:, :N]
        w.copy_(c.w)
        assert w.data_ptr() % 4 == w_off
        y_buf = torch.full((M, N + 5), -7.25, dtype=torch.float32, device="cuda")
        st, _ = raw(lib, c, x=x, lda=lda, w=w, ldw=ldw, y=y_buf, ldy=N + 5)
        assert st == 0, lib.oq_last_error().decode()
        assert same_bytes(y_buf[:, :N].contiguous(), c.want), (lda, offset, w_off, where_wrong(y_buf[:, :N].contiguous(), c.want))
        assert (y_buf[:, N:] == -7.25).all()


def test_a_512_tile_grid_gives_the_same_bytes_four_times(ops):
    M, K, N = 512, 64, 16384
    assert plan(M, K, N).tiles == 512 and plan(M, K, N).splits == 1
    c = QCase(31, M, K, N, "dynamic", "dynamic", gemm=True)
    first = c.call(ops)
    assert same_bytes(first, c.want), where_wrong(first, c.want)
    for _ in range(3):
        assert torch.equal(c.call(ops).view(torch.int32), first.view(torch.int32))


# ------------------------------------------------------------------------------------ 4. the dynamic parameters at their edges
M_E, K_E, N_E = 6, 83, 70                      # the last row ends in a partial chunk of 3 (16-chunks) and of 3 (4-chunks)
PLACES = {"first": (0, 0), "middle": (3, 41), "last": (M_E - 1, K_E - 1), "last partial chunk": (M_E - 1, 80)}


def edge_case(x, gemm=True, out_mode=None):
    return QCase(41, M_E, K_E, N_E, "dynamic", out_mode, gemm=gemm, x=x)


def test_dynamic_input_all_zero_gives_the_bias_exactly(ops):
    c = edge_case(np.zeros((M_E, K_E), F))
    y = c.call(ops)
    B, b_scale, b_zp = c.bias
    bias = (B.cpu().numpy().astype(F) - F(int(b_zp))) * F(float(b_scale))
    assert same_bytes(y, np.broadcast_to(bias, (M_E, N_E)).copy()) and same_bytes(y, c.want)


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["positive", "negative"])
def test_dynamic_input_of_one_sign_clamps_its_range_at_zero(ops, sign):
    x = (sign * np.random.default_rng(3).uniform(0.5, 4.0, (M_E, K_E))).astype(F)
    c = edge_case(x)
    safe, scale, zp = dyn_params(x)
    assert zp == (0 if sign > 0 else 255) and scale == F(np.abs(x).max()) / F(255)
    assert same_bytes(c.call(ops), c.want), where_wrong(c.call(ops), c.want)


@pytest.mark.parametrize("place", sorted(PLACES))
@pytest.mark.parametrize("lda_gap", [0, 1], ids=["vector rows", "narrow rows"])
def test_the_extreme_element_is_found_wherever_it_lies_and_a_nan_poisons_everything(ops, lib, place, lda_gap):
    rng = np.random.default_rng(9)
    for value in (1000.0, -1000.0, float("nan")):
        x = rng.standard_normal((M_E, K_E)).astype(F)
        x[PLACES[place]] = value
        c = edge_case(x, out_mode="dynamic" if np.isnan(value) else None)
        lda = 85 if lda_gap else 84                     # K_E = 83: rows 4-byte aligned only / 16-byte aligned
        buf = torch.full((M_E, lda), 3e38, dtype=torch.float32, device="cuda")
        buf[:, :K_E] = c.x
        st, y = raw(lib, c, x=buf[:, :K_E], lda=lda)
        assert st == 0
        if np.isnan(value):
            assert torch.isnan(y).all()
            for out_mode in (None, "static"):
                st, y = raw(lib, QCase(41, M_E, K_E, N_E, "static", out_mode, gemm=True), x=buf[:, :K_E], lda=lda, x_mode=DYNAMIC)
                assert st == 0 and torch.isnan(y).all(), out_mode
        else:
            assert same_bytes(y, c.want), (value, where_wrong(y, c.want))


@pytest.mark.parametrize("lo,zp", [(-0.5, 0), (-1.5, 2), (-2.5, 2)])
def test_a_tie_in_the_zero_point_goes_to_even(ops, lo, zp):
    x = np.random.default_rng(4).uniform(lo, lo + 255.0, (M_E, K_E)).astype(F)
    x[0, 0], x[1, 1] = lo, lo + 255.0                   # scale = 1 exactly, -lo / safe = n + 0.5
    c = edge_case(x)
    assert dyn_params(x) == (F(1), F(1), F(zp))
    assert same_bytes(c.call(ops), c.want), where_wrong(c.call(ops), c.want)


def planted(M, K, N, row, hot, cold, near_top=False):
    """uint8 levels of X and a uint8 W whose largest sum lies at (row, hot) and whose smallest at (row, cold); `near_top`: every value
    within 3 of the zero points 255 -- small valid sums beside large correction terms -- and no planted minimum."""
    rng = np.random.default_rng(12)
    q = rng.integers(252, 256, (M, K)) if near_top else rng.integers(100, 156, (M, K))
    w = rng.integers(252, 256, (K, N)) if near_top else rng.integers(100, 156, (K, N))
    q[row], w[:, hot] = (240, 240) if near_top else (255, 255)
    if not near_top:
        w[:, cold] = 0
    return q, torch.from_numpy(w.astype(np.uint8)).cuda()


@pytest.mark.parametrize("case", ["first tile", "last tile", "partial tile", "split K"])
def test_the_extreme_v_is_found_wherever_it_lies(ops, case):
    """The (min, max) pairs of the workgroups: the extremes in the first and in the last tile, in a partial tile (one valid row, four
    valid columns) whose padding lanes hold large correction terms, and where the reduce kernel finishes v."""
    M, K, N = (16, 1088, 260) if case == "split K" else (129, 64, 16388)
    assert (plan(M, K, N).splits > 1) == (case == "split K")
    row, hot, cold = (0, 0, 1) if case == "first tile" else (M - 1, N - 1, N - 2)
    near_top = case == "partial tile"
    zp = 255 if near_top else 131                       # zero_point("hi") / ("mid") of uint8
    q, w = planted(M, K, N, row, hot, cold, near_top)
    c = QCase(51, M, K, N, "static", "dynamic", x_dt="u8", w_dt="u8", x_zp="hi" if near_top else "mid", w_zp="hi" if near_top else "mid",
              per_column=False, w=w, x=((q - zp) * 0.0123).astype(F), w_scale=0.01)
    assert int(c.x_zp) == zp == int(c.w_zp)
    assert np.unravel_index(np.argmax(c.v), c.v.shape) == (row, hot)
    if not near_top:
        assert np.unravel_index(np.argmin(c.v), c.v.shape) == (row, cold)
    y = c.call(ops)
    assert same_bytes(y, c.want), where_wrong(y, c.want)


@pytest.mark.parametrize("out_dt", ["u8", "i8"])
def test_static_output_ties_and_saturation(lib, out_dt):
    """x_scale = 2^-5, w_scale = 1, out_scale = 2^-4: v / out_scale = S / 2 exactly, a tie for every odd S; small enough that both
    ends of the output type saturate."""
    c = QCase(61, 33, 40, 130, "static", "static", x_dt="i8", w_dt="i8", x_zp=None, w_zp=None, out_zp="mid", out_dt=out_dt, per_column=False,
              x_scale=2.0 ** -5, w_scale=1.0, out_scale=2.0 ** -4, w=torch.randint(-3, 4, (40, 130), dtype=torch.int8, device="cuda"),
              x=(np.random.default_rng(6).integers(-30, 31, (33, 40)) * 2.0 ** -5).astype(F))
    assert (c.S % 2 != 0).sum() > 100
    lo, hi = RANGE[DT[out_dt]]
    q = c.want / F(2.0 ** -4) + F(int(c.out_zp))
    assert q.min() == lo and q.max() == hi
    st, y = raw(lib, c)
    assert st == 0 and same_bytes(y, c.want), where_wrong(y, c.want)


# ------------------------------------------------------------------------------------ 5. real arithmetic, memory
@pytest.mark.parametrize("x_mode", ["static", "dynamic"])
def test_the_result_is_within_four_roundings_of_real_arithmetic(ops, x_mode):
    """|Y - R| <= 4 * 2^-24 * (|R_product| + |bias|), R in float64 from the same integers and fp32 parameters: the roundings of
    fp32(S), of x_scale * w_scale[n] and of their product, and the one of the bias addition."""
    c = QCase(71, 129, 1088, 260, x_mode, None, gemm=True)
    y = c.call(ops).cpu().numpy().astype(np.float64)
    xs = float(dyn_params(c.x_np)[1]) if x_mode == "dynamic" else float(c.x_scale)
    product = c.S.astype(np.float64) * xs * c.w_scale.cpu().numpy().astype(np.float64).reshape(1, -1)
    B, b_scale, b_zp = c.bias
    bias = (B.cpu().numpy().astype(np.float64) - float(b_zp)) * float(b_scale)
    err = np.abs(y - (product + bias))
    bound = 4 * 2.0 ** -24 * (np.abs(product) + np.abs(bias))
    print("largest error / bound:", float((err / bound).max()))
    assert (err <= bound).all()


def test_peak_memory_of_a_call_is_the_output_and_the_workspace(ops, lib):
    M, K, N = 64, 1024, 1024
    c = QCase(81, M, K, N, "dynamic", "dynamic", gemm=True)
    r512 = lambda n: (n + 511) // 512 * 512      # noqa: E731  (the allocator's granule)
    need = lib.oq_qdq_function_workspace_bytes(M, K, N, MODE["dynamic"], MODE["dynamic"])
    assert need == workspace(M, K, N, DYNAMIC, DYNAMIC)
    c.call(ops)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = c.call(ops)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before == r512(M * N * 4) + r512(need)
    del out


def test_what_the_kernel_leaves_out_is_refused_by_name(ops):
    c = QCase(91, 16, 64, 32, "static", None)
    for over, word in ((dict(x=c.x.half()), "fp32"), (dict(x_mode=None), "x_mode"), (dict(w_scale=torch.ones(64, device="cuda")), "grouped"),
                       (dict(out_mode="static"), "out_scale")):
        kw = dict(c.kwargs(), x=c.x, w=c.w, w_scale=c.w_scale, w_zero_point=c.w_zp)
        kw.update(over)
        x, w, w_scale, w_zp = (kw.pop(k) for k in ("x", "w", "w_scale", "w_zero_point"))
        with pytest.raises(NotImplementedError, match=word):
            ops.qdq_function(x, w, w_scale, w_zp, **kw)
