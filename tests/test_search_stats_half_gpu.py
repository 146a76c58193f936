"""The running statistics of the AWQ / SmoothQuant searches straight from fp16 / bf16 activations (oq_abs_stats_cols_many_h16,
csrc/abs_stats_half.hip; ops.abs_stats_accumulate_many, ops.SearchStatistics, ActivationStream `statistics_names`) against the
route they replace: the fp32 kernels on ``x.float()``.

|x| of a half value is exact and the kernel keeps the summation order of oq_abs_sum_cols_f32 (min(T, 64) row chunks, fours
as (a + b) + (c + d), then single rows, chunks from 0), so `abs_sum` and `absmax` are compared bit for bit.  A lane owns 8, 4, 2
or 1 adjacent columns: 8 and 4 only when the table is large enough to fill the device at that width (16384 / 32768 columns for a
single item), so the shapes below include such widths next to the small ones."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ["float16", "bfloat16"]
ROWS = [1, 3, 4, 5, 63, 64, 65, 67, 130, 257, 1000]      # chunk count, chunk length (1, 2, 3, 5, 16) and the four-row tail
COLS = [1, 7, 8, 9, 256, 257, 520]
WIDE = [(67, 16384), (130, 32768), (850, 32768)]          # 4 and 8 columns per lane; 850 rows: chunks of 14 = 8 in flight + a four + 2


def _dt(name):
    import torch
    return getattr(torch, name)


def _source(dtype, seed=0):
    """One random matrix per element type and seed, made once: the tests slice it."""
    import torch
    key = (dtype, seed)
    if key not in _source.cache:
        g = torch.Generator(device="cuda").manual_seed(1234 + seed)
        _source.cache[key] = (torch.randn(1024, 600, generator=g, device="cuda") * 3.0).to(_dt(dtype))
    return _source.cache[key]


_source.cache = {}


def _layouts(base):
    """`base` [T, K] in three row layouts: contiguous; an odd leading dimension (a column slice of a wider matrix); a base at an
    odd element offset."""
    import torch
    t, k = base.shape
    width = k + 1 if k % 2 == 0 else k + 2
    wide = torch.zeros(t, width, dtype=base.dtype, device="cuda")
    wide[:, :k] = base
    flat = torch.zeros(t * k + 1, dtype=base.dtype, device="cuda")
    flat[1:] = base.reshape(-1)
    odd_base = flat[1:].view(t, k)
    assert wide[:, :k].stride(0) % 2 == 1 and odd_base.data_ptr() % 4 == 2
    return {"contiguous": base.contiguous(), "odd ldx": wide[:, :k], "odd base": odd_base}


def _running(k, seed=0):
    """Non-zero running values: some maxima above what a batch of N(0, 3) brings, some below."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(99 + seed)
    return (torch.rand(k, generator=g, device="cuda") * 50.0 + 0.5, torch.rand(k, generator=g, device="cuda") * 12.0)


def _fp32_route(x, abs_sum, absmax):
    """What the parent commit computed for one tensor: the cast, oq_abs_sum_cols_f32 accumulating, oq_absmax_f32, torch.maximum.
    Returns the new absmax (abs_sum is updated in place)."""
    import torch
    from onnx_quantize_amd.hip import _lib as L
    from onnx_quantize_amd.hip import ops
    x2 = x.float().reshape(-1, x.shape[-1]).contiguous()
    t, k = x2.shape
    lib = L.load()
    ws = torch.empty(lib.oq_abs_sum_cols_workspace_bytes(k), dtype=torch.uint8, device="cuda")
    L.check(lib.oq_abs_sum_cols_f32(x2.data_ptr(), t, k, k, abs_sum.data_ptr(), 1, ws.data_ptr(), ws.numel(), None))
    return torch.maximum(absmax, ops.absmax(x2))


def _same_bits(a, b):
    import torch
    return a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _same_values(a, b):
    """`_same_bits` where a NaN equals a NaN, whatever its payload."""
    import torch
    nan = torch.isnan(a)
    return torch.equal(nan, torch.isnan(b)) and _same_bits(a[~nan], b[~nan])


def _stats(k, running=None):
    from onnx_quantize_amd.hip import ops
    st = ops.SearchStatistics(k, "cuda")
    if running is not None:
        st.abs_sum.copy_(running[0])
        st.absmax.copy_(running[1])
    return st


# ------------------------------------------------------------------------------------ bit-equality with the fp32 route
@pytest.mark.parametrize("dtype", DTYPES)
def test_statistics_are_bit_equal_to_the_fp32_route(dtype):
    """Two SearchStatistics from the same non-zero running values, one fed x, one fed x.float()."""
    import torch
    src, bad = _source(dtype), []
    for k in COLS:
        running = _running(k)
        for t in ROWS:
            for name, x in _layouts(src[:t, :k]).items():
                got, ref = _stats(k, running), _stats(k, running)
                got.add(x)
                ref.add(x.float())
                if not (_same_bits(got.abs_sum, ref.abs_sum) and _same_bits(got.absmax, ref.absmax) and got.rows == ref.rows == t):
                    bad.append((t, k, name, (got.abs_sum - ref.abs_sum).abs().max().item()))
    assert not bad, bad[:8]
    assert got.gram.dtype == torch.float32


@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_items_take_the_wide_loads_and_give_the_same_bits(dtype):
    """16384 / 32768 columns: the widths at which a single item runs 4 / 8 columns per lane (no Gram matrix of that width is made:
    the op is called directly).  Aligned rows, and rows that force the narrow loads on the same data."""
    import torch
    from onnx_quantize_amd.hip import ops
    g = torch.Generator(device="cuda").manual_seed(7)
    bad = []
    for t, k in WIDE:
        base = (torch.randn(t, k, generator=g, device="cuda") * 3.0).to(_dt(dtype))
        for name, x in _layouts(base).items():
            abs_sum, absmax = (v.clone() for v in _running(k, 1))
            ref_sum, ref_max = (v.clone() for v in _running(k, 1))
            ops.abs_stats_accumulate_many([x], [abs_sum], [absmax])
            ref_max = _fp32_route(x, ref_sum, ref_max)
            if not (_same_bits(abs_sum, ref_sum) and _same_bits(absmax, ref_max)):
                bad.append((t, k, name))
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_three_batch_sequence_stays_equal_throughout(dtype):
    src = _source(dtype, 1)
    for k in (9, 520):
        got, ref = _stats(k, _running(k, 2)), _stats(k, _running(k, 2))
        row = 0
        for t in (5, 257, 130):
            x = src[row:row + t, :k]
            row += t
            got.add(x)
            ref.add(x.float())
            assert _same_bits(got.abs_sum, ref.abs_sum) and _same_bits(got.absmax, ref.absmax) and got.rows == ref.rows == row, (k, t)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_3d_input_equals_its_flattened_form(dtype):
    import torch
    x = _source(dtype, 1)[:650, :520].contiguous().reshape(5, 130, 520)
    a, b = _stats(520), _stats(520)
    a.add(x)
    b.add(x.reshape(650, 520))
    assert _same_bits(a.abs_sum, b.abs_sum) and _same_bits(a.absmax, b.absmax) and a.rows == b.rows == 650    # rows count as samples
    assert torch.equal(a.gram, b.gram)


# ------------------------------------------------------------------------------------ independent of the fp32 kernel
@pytest.mark.parametrize("dtype", DTYPES)
def test_statistics_against_float64_and_torch(dtype):
    """All terms are non-negative, so every fp32 add contributes at most one rounding of relative 2^-24 to the sum; a column takes
    fewer than T + 64 adds (rows, chunk sums, the running value)."""
    import torch
    from onnx_quantize_amd.hip import ops
    src = _source(dtype)
    cases = [src[:t, :k] for t in (1, 5, 67, 1000) for k in (1, 9, 520)]
    g = torch.Generator(device="cuda").manual_seed(3)
    cases += [(torch.randn(t, k, generator=g, device="cuda") * 3.0).to(_dt(dtype)) for t, k in WIDE]
    for x in cases:
        t, k = x.shape
        abs_sum, absmax = torch.zeros(k, device="cuda"), torch.zeros(k, device="cuda")
        ops.abs_stats_accumulate_many([x], [abs_sum], [absmax])
        want = x.double().abs().sum(0)
        err = ((abs_sum.double() - want).abs() / want.clamp_min(1e-300)).max().item()
        print(f"{dtype} T={t} K={k}: max relative error of abs_sum {err:.3e}, bound {(t + 64) * 2.0 ** -24:.3e}")
        assert err <= (t + 64) * 2.0 ** -24, (t, k, err)
        assert torch.equal(absmax, x.float().abs().amax(0)), (t, k)


# ------------------------------------------------------------------------------------ special values
def _special_positions(t):
    """Rows at the head, in the body (the four behind the loads in flight) and in the tail (the single rows) of chunk 3."""
    per = -(-t // min(t, 64))
    first = 3 * per
    return {"head": first, "body": first + per - 1 - (per % 4) - 1, "tail": first + per - 1}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("t,k", [(1350, 24), (1350, 7), (850, 32768)], ids=["two per lane", "one per lane", "eight per lane"])
def test_special_values_in_the_head_body_and_tail_of_a_chunk(dtype, t, k):
    """1350 rows: chunks of 22 = 16 loads in flight + one four + 2 single rows; 850 rows: chunks of 14 = 8 + 4 + 2."""
    import torch
    from onnx_quantize_amd.hip import ops
    dt = _dt(dtype)
    g = torch.Generator(device="cuda").manual_seed(11)
    clean = (torch.randn(t, k, generator=g, device="cuda") * 3.0).to(dt)
    pos = _special_positions(t)
    assert pos["head"] < pos["body"] < pos["tail"] and (pos["tail"] + 1) % (-(-t // 64)) == 0

    def run(x):
        abs_sum, absmax = torch.zeros(k, device="cuda"), torch.zeros(k, device="cuda")
        ops.abs_stats_accumulate_many([x], [abs_sum], [absmax])
        ref_sum = torch.zeros(k, device="cuda")
        ref_max = _fp32_route(x, ref_sum, torch.zeros(k, device="cuda"))
        assert _same_values(abs_sum, ref_sum) and _same_values(absmax, ref_max)
        return abs_sum, absmax

    clean_sum, clean_max = run(clean)
    cols = torch.arange(k, device="cuda")
    big = 65504.0 if dtype == "float16" else 3.39e38
    tiny = 2.0 ** -24 if dtype == "float16" else 2.0 ** -133          # subnormal in either format
    for where, row in pos.items():
        col = (5 * row + 3) % k
        keep = cols != col
        for value in (float("nan"), float("inf"), float("-inf")):
            x = clean.clone()
            x[row, col] = value
            s, m = run(x)
            if value != value:
                assert torch.isnan(s[col]) and torch.isnan(m[col]), where
            else:
                assert s[col] == float("inf") and m[col] == float("inf"), (where, value)
            assert torch.equal(s[keep], clean_sum[keep]) and torch.equal(m[keep], clean_max[keep]), (where, value)    # exactly its column
        x = clean.clone()                       # a column of -0 with one subnormal: +0 comes out, the subnormal is a value
        x[:, col] = -0.0
        s, m = run(x)
        assert s[col].view(torch.int32) == 0 and m[col].view(torch.int32) == 0, where
        x[row, col] = -tiny
        s, m = run(x)
        assert s[col] == tiny and m[col] == tiny, where
        x = clean.clone()                       # the largest finite value twice in one column: the bf16 sum overflows, as the fp32 route's
        x[:, col] = 0.0
        x[row, col] = big
        x[pos["head"] + 1, col] = -big
        s, m = run(x)
        assert m[col] == torch.tensor(big, dtype=dt).float()
        assert (s[col] == float("inf")) if dtype == "bfloat16" else (s[col] == 2 * 65504.0), (where, s[col])
    # a NaN in the running value stays
    abs_sum, absmax = torch.zeros(k, device="cuda"), torch.zeros(k, device="cuda")
    abs_sum[1 % k] = float("nan")
    absmax[2 % k] = float("nan")
    ops.abs_stats_accumulate_many([clean], [abs_sum], [absmax])
    assert torch.isnan(abs_sum[1 % k]) and torch.isnan(absmax[2 % k]) and int(torch.isnan(abs_sum).sum() + torch.isnan(absmax).sum()) == 2


# ------------------------------------------------------------------------------------ lists
def _five_items(dtype):
    """Five items that differ in T and K and take 8, 1, 2, 4 and 1 columns per lane in one table (the wide first item makes the table
    large enough for 8): 16-byte aligned rows; K odd; a base 4 bytes past a 16-byte boundary; a base 8 bytes past one; an odd
    leading dimension taken from an odd element offset."""
    import torch
    dt = _dt(dtype)
    g = torch.Generator(device="cuda").manual_seed(21)

    def rnd(*shape):
        return (torch.randn(*shape, generator=g, device="cuda") * 3.0).to(dt)

    a = rnd(130, 32768)
    b = rnd(257, 257)
    c = rnd(5 * 1028 + 8)[2:2 + 5 * 1028].view(5, 1028)
    d = rnd(64 * 256 + 8)[4:4 + 64 * 256].view(64, 256)
    e = rnd(1000 * 11 + 8)[1:1 + 1000 * 11].view(1000, 11)[:, :9]
    assert a.data_ptr() % 16 == 0 and c.data_ptr() % 16 == 4 and d.data_ptr() % 16 == 8 and e.data_ptr() % 4 == 2 and e.stride(0) == 11
    return [a, b, c, d, e]


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_call_on_a_table_equals_a_call_per_item(dtype):
    from onnx_quantize_amd.hip import ops
    xs = _five_items(dtype)
    many = [tuple(v.clone() for v in _running(x.shape[1], i)) for i, x in enumerate(xs)]
    single = [tuple(v.clone() for v in _running(x.shape[1], i)) for i, x in enumerate(xs)]
    ops.abs_stats_accumulate_many(xs, [m[0] for m in many], [m[1] for m in many])
    for x, (s, m) in zip(xs, single):
        ops.abs_stats_accumulate_many([x], [s], [m])                       # count = 1: no device table
    for i, (x, got, one) in enumerate(zip(xs, many, single)):
        assert _same_bits(got[0], one[0]) and _same_bits(got[1], one[1]), (i, tuple(x.shape))
        ref_sum, ref_max = (v.clone() for v in _running(x.shape[1], i))
        ref_max = _fp32_route(x, ref_sum, ref_max)
        assert _same_bits(got[0], ref_sum) and _same_bits(got[1], ref_max), (i, tuple(x.shape))


@pytest.mark.parametrize("dtype", DTYPES)
def test_count_one_with_a_null_device_table(dtype):
    """The C call itself: the item is read from the host copy."""
    import torch
    from onnx_quantize_amd.hip import _lib as L
    x = _source(dtype)[:257, :520].contiguous()
    abs_sum, absmax = (v.clone() for v in _running(520, 5))
    ref_sum, ref_max = (v.clone() for v in _running(520, 5))
    lib = L.load()
    host = np.asarray([[x.data_ptr(), 257, 520, 520, abs_sum.data_ptr(), absmax.data_ptr()]], dtype=np.int64)
    hp = C.c_void_p(host.ctypes.data)
    need = lib.oq_abs_stats_many_half_workspace_bytes(hp, 1)
    assert need == 64 * 520 * 8 + 256
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    L.check(lib.oq_abs_stats_cols_many_h16(hp, None, 1, L.WTYPE_CODE[dtype], ws.data_ptr(), need, None))
    ref_max = _fp32_route(x, ref_sum, ref_max)
    assert _same_bits(abs_sum, ref_sum) and _same_bits(absmax, ref_max)


def test_a_mixed_add_many_equals_per_tensor_adds():
    """fp32, fp16 and bf16 values of one batch: `abs_sum`, `absmax` and `rows` are those of per-tensor `add` calls, and every Gram
    matrix is the bits of the tensor's own `hessian_accumulate` (which `add` runs).  Two half items per type are large enough for
    the grouped Hessian chain (>= 512 rows and columns) and stay within the 992 rows up to which that chain gives the per-tensor
    bits; the fp32 items are below the grouping threshold, where both routes run the per-tensor call (the grouped fp32 chain is a
    different Hessian method and not this test's subject)."""
    import torch
    from onnx_quantize_amd.hip import ops
    f16, bf16 = _source("float16", 2), _source("bfloat16", 2)
    xs = [f16[:300, :256].float(), f16[:600, :512], bf16[:512, :512], f16[:5, :24], bf16[:700, :520].contiguous().reshape(7, 100, 520),
          f16[100:620, :600], bf16[:64, :9].float(), bf16[3:70, :257]]
    many = [_stats(x.shape[-1], _running(x.shape[-1], i)) for i, x in enumerate(xs)]
    single = [_stats(x.shape[-1], _running(x.shape[-1], i)) for i, x in enumerate(xs)]
    for st in many + single:
        st.rows = 3
        st.gram.fill_diagonal_(0.25)
    ops.SearchStatistics.add_many(many, xs)
    for st, x in zip(single, xs):
        st.add(x)
    for i, (a, b, x) in enumerate(zip(many, single, xs)):
        assert _same_bits(a.abs_sum, b.abs_sum) and _same_bits(a.absmax, b.absmax), (i, x.dtype, tuple(x.shape))
        assert a.rows == b.rows == 3 + x.numel() // x.shape[-1], i
        assert torch.equal(a.gram, b.gram), (i, x.dtype, tuple(x.shape))


# ------------------------------------------------------------------------------------ the searches
SEARCHES = [("uint4", "group", 32, False), ("int8", "channel", -1, True), ("uint8", "tensor", -1, False), ("int4", "group", 128, False),
            ("int8", "group", 8, False)]


def _search_inputs(dtype):
    """tests/test_preprocessing.py::_inputs(5, 768, 256, 192), the activations rounded to the half type; made once per type."""
    import torch
    if dtype not in _search_inputs.cache:
        r = np.random.default_rng(5)
        x = r.standard_normal((4, 192, 256)).astype(np.float32) * r.uniform(0.1, 4, 256).astype(np.float32)
        w = (r.standard_normal((256, 192)) * 0.05).astype(np.float32)
        xh = torch.from_numpy(x).cuda().to(_dt(dtype)).reshape(768, 256)
        _search_inputs.cache[dtype] = (xh, xh.float().cpu().numpy(), torch.from_numpy(w).cuda(), w)
    return _search_inputs.cache[dtype]


_search_inputs.cache = {}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("qtype,strategy,g,sym", SEARCHES)
def test_searches_from_half_statistics_follow_the_oracle(dtype, qtype, strategy, g, sym):
    """The bars of test_gpu_searches_from_streamed_statistics_follow_the_oracle, the oracle run on the upcast concatenation."""
    import oq_oracle as O
    import torch
    from onnx_quantize_amd.hip import ops
    xh, x, wd, w = _search_inputs(dtype)
    stats = ops.SearchStatistics(256, "cuda")
    for part in (xh[:1], xh[1:3], xh[3:]):                                  # three uneven batches
        stats.add(part)
    assert stats.rows == 768
    es, el = O.awq_scale_search(x, w, qtype, strategy, g, sym)
    s, l = ops.awq_scale_search_stats(stats, wd, qtype, strategy, g, sym)
    np.testing.assert_allclose(l, el, rtol=2e-3)
    assert el[int(np.argmin(l))] <= el.min() * (1 + 2e-3)
    if int(np.argmin(l)) == int(np.argmin(el)):
        np.testing.assert_allclose(s.cpu().numpy(), es, rtol=2e-5)
    er, ecl = O.awq_clip_search(x, w, qtype, strategy, g, sym)
    r, cl = ops.awq_clip_search_stats(stats, wd, qtype, strategy, g, sym)
    np.testing.assert_allclose(cl, ecl, rtol=2e-3)
    assert ecl[int(round((1 - r) * 100))] <= ecl.min() * (1 + 2e-3)
    assert torch.equal(ops.smooth_quant_scale_stats(stats, wd, 0.5), ops.smooth_quant_scale(xh.float(), wd, 0.5))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_half_weight_gives_the_bits_of_its_upcast(dtype):
    import torch
    from onnx_quantize_amd.hip import ops
    xh, _, wd, _ = _search_inputs(dtype)
    stats = ops.SearchStatistics(256, "cuda")
    stats.add(xh)
    for wdt in (torch.float16, torch.bfloat16):
        wh = wd.to(wdt)
        s, l = ops.awq_scale_search_stats(stats, wh, "uint4", "group", 32)
        s2, l2 = ops.awq_scale_search_stats(stats, wh.float(), "uint4", "group", 32)
        assert torch.equal(s, s2) and np.array_equal(l, l2)
        r, cl = ops.awq_clip_search_stats(stats, wh, "uint4", "group", 32)
        r2, cl2 = ops.awq_clip_search_stats(stats, wh.float(), "uint4", "group", 32)
        assert r == r2 and np.array_equal(cl, cl2)
        assert torch.equal(ops.smooth_quant_scale_stats(stats, wh, 0.5), ops.smooth_quant_scale_stats(stats, wh.float(), 0.5))
        assert torch.equal(ops.smooth_quant_scale(xh.float(), wh, 0.5), ops.smooth_quant_scale(xh.float(), wh.float(), 0.5))


# ------------------------------------------------------------------------------------ no fp32 copy
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_fp32_copy_of_the_activation_is_made(dtype):
    """A 4096 x 1024 half tensor is 8 MB; its fp32 copy would be 16 MB.  After a warm call (the workspaces of the Hessian kernels
    exist from then on) `add` allocates the 0.5 MB of partial sums and maxima."""
    import torch
    x = _source(dtype).repeat(4, 2)[:, :1024].contiguous()
    assert x.shape == (4096, 1024) and x.dtype == _dt(dtype)
    stats = _stats(1024)
    stats.add(x)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    stats.add(x)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert rise < x.numel() * 4, rise
    assert stats.rows == 8192 and torch.equal(stats.absmax, x.float().abs().amax(0))


# ------------------------------------------------------------------------------------ the driver
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_driver_folds_half_statistics_names_as_they_arrive(dtype):
    import torch
    from onnx_quantize_amd import calibration_driver as D
    from onnx_quantize_amd.hip import ops
    torch.manual_seed(4)
    model = torch.nn.Sequential()
    model.add_module("fc1", torch.nn.Linear(40, 72))
    model.add_module("act", torch.nn.ReLU())
    model.add_module("fc2", torch.nn.Linear(72, 24))
    model = model.cuda().to(_dt(dtype))
    taps = {"X": ("fc1", "input"), "a1": ("fc2", "input")}
    data = (torch.randn(40, 7, 40) * 2).to(_dt(dtype))
    runner = D.TorchRunner(model, taps)
    seen = []

    def recording(feed):
        out = runner(feed)
        seen.append(out)
        return out

    native = D.run_calibration(recording, data, D.ActivationStream(statistics_names=["X", "a1"]), num_samples=40, batch_size=10)
    runner.close()
    assert native.batches == 4 and all(t.dtype == _dt(dtype) for b in seen for t in b.values())
    upcast = D.ActivationStream(statistics_names=["X", "a1"], statistics_after_bytes=0)
    for b in seen:
        upcast.feed({n: t.float() for n, t in b.items()})
    for name, k in (("X", 40), ("a1", 72)):
        got, ref = native.search_input(name), upcast.search_input(name)
        assert isinstance(got, ops.SearchStatistics) and isinstance(ref, ops.SearchStatistics), name      # never held, whatever the threshold
        assert got is native.search_input(name)
        assert _same_bits(got.abs_sum, ref.abs_sum) and _same_bits(got.absmax, ref.absmax) and got.rows == ref.rows == 280, name
        assert got.gram.shape == (k, k)
        assert (got.gram - ref.gram).abs().max() <= 1e-5 * ref.gram.abs().max(), name
    # the searches run on what the stream hands out, with the model's own half weight
    w = model.fc2.weight.detach().t()
    s, losses = ops.awq_scale_search_stats(native.search_input("a1"), w, "uint4", "group", 8)
    assert s.shape == (72,) and np.isfinite(losses).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_fp32_names_are_still_held_next_to_half_names(dtype):
    import torch
    from onnx_quantize_amd import calibration_driver as D
    from onnx_quantize_amd.hip import ops
    src = _source(dtype, 3)
    batches = [{"h": src[i * 60:(i + 1) * 60, :72].reshape(6, 10, 72), "f": src[i * 60:(i + 1) * 60, 100:140].float().reshape(6, 10, 40)} for i in range(3)]
    mixed, alone = D.ActivationStream(statistics_names=["h", "f"]), D.ActivationStream(statistics_names=["f"])
    for b in batches:
        mixed.feed(b)
        alone.feed({"f": b["f"]})
    held = mixed.search_input("f")
    assert isinstance(held, torch.Tensor) and held.dtype == torch.float32
    assert torch.equal(held, torch.cat([b["f"] for b in batches], dim=0)) and torch.equal(held, alone.search_input("f"))
    h = mixed.search_input("h")
    assert isinstance(h, ops.SearchStatistics) and h.rows == 180
    # past the threshold the fp32 name folds exactly as it does without the half name
    mixed, alone = (D.ActivationStream(statistics_names=n, statistics_after_bytes=20000) for n in (["h", "f"], ["f"]))
    for b in batches:
        mixed.feed(b)
        alone.feed({"f": b["f"]})
    a, b = mixed.search_input("f"), alone.search_input("f")
    assert isinstance(a, ops.SearchStatistics) and isinstance(b, ops.SearchStatistics)
    assert _same_bits(a.abs_sum, b.abs_sum) and _same_bits(a.absmax, b.absmax) and a.rows == b.rows == 180 and torch.equal(a.gram, b.gram)


# ------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_refused_table_leaves_every_output_untouched(dtype):
    import torch
    from onnx_quantize_amd.hip import _lib as L
    from onnx_quantize_amd.hip import ops
    xs = [_source(dtype)[:67, :24].contiguous(), _source(dtype)[:130, :9].contiguous()]
    outs = [tuple(v.clone() for v in _running(x.shape[1], i)) for i, x in enumerate(xs)]
    before = [(s.clone(), m.clone()) for s, m in outs]
    lib = L.load()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    good = [[x.data_ptr(), x.shape[0], x.shape[1], x.shape[1], s.data_ptr(), m.data_ptr()] for x, (s, m) in zip(xs, outs)]
    for what, field, value, status, word in (("ldx < K", 3, 8, -1, "item 1"), ("T = 0", 1, 0, -1, "item 1"), ("null absmax", 5, 0, -1, "item 1")):
        rows = [list(r) for r in good]
        rows[1][field] = value
        host = np.asarray(rows, dtype=np.int64)
        dev = torch.from_numpy(host).cuda()
        st = lib.oq_abs_stats_cols_many_h16(C.c_void_p(host.ctypes.data), dev.data_ptr(), 2, L.WTYPE_CODE[dtype], ws.data_ptr(), ws.numel(), None)
        assert st == status and word in lib.oq_last_error().decode(), (what, st, lib.oq_last_error())
    host = np.asarray(good, dtype=np.int64)
    dev = torch.from_numpy(host).cuda()
    need = lib.oq_abs_stats_many_half_workspace_bytes(C.c_void_p(host.ctypes.data), 2)
    st = lib.oq_abs_stats_cols_many_h16(C.c_void_p(host.ctypes.data), dev.data_ptr(), 2, L.WTYPE_CODE[dtype], ws.data_ptr(), need - 1, None)
    assert st == L.OQ_ERR_WORKSPACE
    st = lib.oq_abs_stats_cols_many_h16(C.c_void_p(host.ctypes.data), dev.data_ptr(), 2, 2, ws.data_ptr(), ws.numel(), None)
    assert st == L.OQ_ERR_INVALID_ARGUMENT
    other = torch.float16 if dtype == "bfloat16" else torch.bfloat16
    with pytest.raises(TypeError) as err:
        ops.abs_stats_accumulate_many([xs[0], xs[1].to(other)], [o[0] for o in outs], [o[1] for o in outs])
    assert "torch.float16" in str(err.value) and "torch.bfloat16" in str(err.value)
    with pytest.raises(TypeError):
        ops.abs_stats_accumulate_many([xs[0].float()], [outs[0][0]], [outs[0][1]])
    with pytest.raises(ValueError):
        ops.abs_stats_accumulate_many(xs, [o[0] for o in outs], [outs[0][1], outs[1][1][:5]])
    torch.cuda.synchronize()
    for (s, m), (s0, m0) in zip(outs, before):
        assert _same_bits(s, s0) and _same_bits(m, m0)
