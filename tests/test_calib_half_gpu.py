"""Calibration ranges and absmax straight from fp16 / bf16 activations (oq_minmax_collect_h16, oq_minmax_collect_many_h16,
oq_absmax_h16; csrc/reduce_half.hip) against the path they replace: the fp32 entry points on ``x.float()``, and torch's own
min / max / abs().amax().  Min, max and |x| of half values are exact, so every comparison is bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ["float16", "bfloat16"]


def _dt(name):
    import torch
    return getattr(torch, name)


def _bits(state):
    """(min bits, max bits, seen bits) of a calibrator state."""
    import torch
    return state[:3].view(torch.int32).tolist()


def _view(count, offset, dtype, seed=0, scale=3.0):
    """`count` random elements starting `offset` elements into a larger buffer: base address 2 * offset bytes past a 16-byte boundary."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed * 1000003 + count * 8 + offset)
    buf = (torch.randn(count + 16, generator=g, device="cuda") * scale).to(dtype)
    x = buf[offset:offset + count]
    assert x.data_ptr() % 16 == (2 * offset) % 16
    return x


def _native(x, momentum=0.0, state=None):
    from onnx_quantize_amd.hip import ops
    state = ops.minmax_state(x.device) if state is None else state
    ops.minmax_collect(x, state, momentum)
    return state


def _reference(x, momentum=0.0, state=None):
    """What the parent commit computed: the cast, then the fp32 kernel."""
    from onnx_quantize_amd.hip import ops
    state = ops.minmax_state(x.device) if state is None else state
    ops.minmax_collect(x.float(), state, momentum)
    return state


# 1 .. 9: head / one vector / tail only; 4095: the one-at-a-time body loop; 32768 + 5: the first count whose body fills one
# eight-deep round of a 512-lane block at every offset; 65536 + 11: two blocks (a block is added per 32768 elements);
# 1 000 003: 30 blocks, several eight-deep rounds and a ragged rest
COUNTS = [1, 7, 8, 9, 4095, 32768 + 5, 65536 + 11, 1_000_003]


@pytest.mark.parametrize("dtype", DTYPES)
def test_state_is_bit_equal_to_the_fp32_path_at_every_alignment(dtype):
    import torch
    bad = []
    for count in COUNTS:
        for offset in range(8):
            x = _view(count, offset, _dt(dtype))
            got, ref = _native(x), _reference(x)
            xf = x.float()
            if _bits(got) != _bits(ref) or got[0] != xf.min() or got[1] != xf.max() or got[2] != 1.0:
                bad.append((count, offset, got.tolist(), ref.tolist()))
    assert not bad, bad[:5]
    assert got.dtype == torch.float32


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_position_counts(dtype):
    """count = 41 at offset 3: five head elements, four vectors, four tail elements."""
    import torch
    base = torch.zeros(64, dtype=_dt(dtype), device="cuda")
    for p in range(41):
        for value in (3.0, -3.0):
            base.zero_()
            x = base[3:44]
            x[p] = value
            st = _native(x).tolist()
            assert st[:2] == ([0.0, 3.0] if value > 0 else [-3.0, 0.0]), (p, value, st)


# count = 100 at offset 3: head = elements 0..4, body = 5..92 (11 vectors), tail = 93..99; 40000 elements reach the eight-deep loop
PLACES = [(100, 2), (100, 50), (100, 97), (100, 99), (40000, 20000)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_anywhere_makes_both_extrema_nan(dtype):
    import torch
    for count, p in PLACES:
        x = _view(count, 3, _dt(dtype))
        x[p] = float("nan")
        got, ref = _native(x), _reference(x)
        assert torch.isnan(got[:2]).all() and torch.isnan(ref[:2]).all() and got[2] == 1.0, (count, p, got.tolist())


@pytest.mark.parametrize("dtype", DTYPES)
def test_infinities_signed_zeros_subnormals_and_the_largest_values(dtype):
    import torch
    dt = _dt(dtype)
    one = torch.tensor([1, -32767], dtype=torch.int16, device="cuda").view(dt)    # bits 0x0001, 0x8001: +- the smallest subnormal, 2^-24 / 2^-133
    tiny = float(one[0].float())
    assert float(one[1].float()) == -tiny
    assert tiny == (2.0 ** -24 if dtype == "float16" else 2.0 ** -133)
    largest = torch.finfo(dt).max                                                  # 65504 / 3.3895e38
    assert largest == (65504.0 if dtype == "float16" else float(np.float32(2.0 ** 127 * (2 - 2.0 ** -7))))
    neg_zero, pos_zero = np.float32(-0.0).view(np.int32).item(), 0
    for count, p in PLACES:
        for value in (float("inf"), float("-inf"), largest, -largest):
            x = _view(count, 3, dt)
            x[p] = value
            got, ref = _native(x), _reference(x)
            assert _bits(got) == _bits(ref) and got[0 if value < 0 else 1] == value, (count, p, value, got.tolist())
        # one -0 among +0: the minimum is -0; one +0 among -0: the maximum is +0
        x = _view(count, 3, dt).zero_()
        x[p] = -0.0
        got = _native(x)
        assert _bits(got)[:2] == [neg_zero, pos_zero] == _bits(_reference(x))[:2], (count, p, _bits(got))
        x = _view(count, 3, dt).zero_().neg_()
        assert _bits(_native(x))[:2] == [neg_zero, neg_zero]
        x[p] = 0.0
        got = _native(x)
        assert _bits(got)[:2] == [neg_zero, pos_zero] == _bits(_reference(x))[:2], (count, p, _bits(got))
        # a subnormal is a value: the smallest magnitude among ones
        x = _view(count, 3, dt).fill_(1.0)
        x[p] = one[0]
        got = _native(x)
        assert _bits(got) == _bits(_reference(x)) and got.tolist()[:2] == [tiny, 1.0], (count, p, got.tolist())
        x = _view(count, 3, dt).fill_(-1.0)
        x[p] = one[1]
        got = _native(x)
        assert _bits(got) == _bits(_reference(x)) and got.tolist()[:2] == [-1.0, -tiny], (count, p, got.tolist())
    # mixed zeros all over
    x = _view(4099, 5, dt).zero_()
    x[::3] = -0.0
    assert _bits(_native(x))[:2] == [neg_zero, pos_zero]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("momentum", [0.0, 0.8])
def test_a_sequence_of_batches_stays_bit_equal(dtype, momentum):
    got = ref = None
    for i, (count, offset) in enumerate([(5000, 1), (70001, 2), (33, 7), (40000, 0)]):
        x = _view(count, offset, _dt(dtype), seed=i + 1, scale=1.0 + i)
        got, ref = _native(x, momentum, got), _reference(x, momentum, ref)
        assert _bits(got) == _bits(ref), (i, got.tolist(), ref.tolist())


@pytest.mark.parametrize("momentum", [0.0, 0.8])
def test_collect_many_on_a_mixed_batch_equals_per_tensor_collect_of_the_upcasts(momentum):
    import torch
    from onnx_quantize_amd.calibration import MinMaxCalibrator
    many, single = MinMaxCalibrator(momentum), MinMaxCalibrator(momentum)
    f16, bf16 = torch.float16, torch.bfloat16
    for b in range(3):
        batch = {
            "f32": torch.randn(3, 1001, device="cuda") * (b + 1),
            "f16.ragged": _view(70001, 1, f16, seed=10 + b),
            # 64 slices of 512 lanes x 8 loads x 8 elements = 2 097 152: these enter the eight-deep round of the list kernel
            "f16.large": _view(2_100_003, 3, f16, seed=15 + b),
            "bf16.large": _view(2_100_003, 6, bf16, seed=45 + b),
            "f16.tiny": _view(3, 5, f16, seed=20 + b),
            "f16.rows": _view(2 * 333 * 65, 0, f16, seed=30 + b).reshape(2, 333, 65)[:, 1:, :],   # an unaligned view
            "bf16.ragged": _view(40009, 7, bf16, seed=40 + b),
            "bf16.tiny": _view(3, 2, bf16, seed=50 + b),
            "bf16.strided": _view(515 * 1030, 0, bf16, seed=60 + b).reshape(515, 1030)[:, 1:1022],     # made contiguous on the way
        }
        if b != 1:
            batch["f16.sometimes"] = _view(777, 3, f16, seed=70 + b)
            batch["bf16.sometimes"] = _view(4097, 4, bf16, seed=80 + b)
        many.collect_many(batch)
        for name, t in batch.items():
            single.collect(name, t.float())
        assert many.data.keys() == single.data.keys()
        for name in single.data:
            a, r = many.data[name]._state, single.data[name]._state
            assert a.dtype == torch.float32 and _bits(a) == _bits(r), (b, name, a.tolist(), r.tolist())
            assert many.data[name]._np_dtype == np.float32
    lo, hi = many.compute_range("bf16.ragged")
    assert lo.dtype == np.float32 and hi.dtype == np.float32


def test_dtype_rules_of_the_ops():
    import torch
    from onnx_quantize_amd.hip import ops
    x = torch.ones(64, dtype=torch.float16, device="cuda")
    with pytest.raises(TypeError, match="fp32"):
        ops.minmax_collect(x, ops.minmax_state(x.device, torch.float64))
    with pytest.raises(TypeError, match="one dtype"):
        ops.minmax_collect_many([x, x.bfloat16()], [ops.minmax_state(x.device), ops.minmax_state(x.device)])
    with pytest.raises(TypeError):
        ops.minmax_collect_many([x], [ops.minmax_state(x.device, torch.float64)])
    with pytest.raises(TypeError):
        ops.minmax_collect(x.cpu(), ops.minmax_state(x.device))


# ------------------------------------------------------------------------------------ absmax
def _absmax_cases(dt):
    import torch
    g = torch.Generator(device="cuda").manual_seed(11)
    rand = lambda *s: (torch.randn(*s, generator=g, device="cuda") * 4).to(dt)          # noqa: E731
    w = rand(515, 1030)
    v = rand(257, 1040)
    return {"[6,333,644]": rand(6, 333, 644), "[515,1030]": w, "w[:,1:1022]": w[:, 1:1022], "C=1": rand(300, 1), "R=1": rand(1, 777),
            "[257,1032] 16-byte rows": rand(257, 1032), "v[:,8:1032] 16-byte rows, ldx 1040": v[:, 8:1032], "[3,8]": rand(3, 8)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("per_row", [False, True], ids=["columns", "rows"])
def test_absmax_equals_torch_and_the_fp32_kernel(dtype, per_row):
    import torch
    from onnx_quantize_amd.hip import ops
    for name, x in _absmax_cases(_dt(dtype)).items():
        if per_row and x.dim() != 2:
            x = x.reshape(-1, x.shape[-1])
        got = ops.absmax(x, per_row=per_row)
        x2 = x.float().reshape(-1, x.shape[-1])
        assert got.dtype == torch.float32 and got.shape == (x2.shape[0] if per_row else x2.shape[1],)
        assert torch.equal(got, x2.abs().amax(1 if per_row else 0)), name
        assert torch.equal(got, ops.absmax(x.float(), per_row=per_row)), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_absmax_nan_poisons_exactly_its_column_or_row(dtype):
    import torch
    from onnx_quantize_amd.hip import ops
    for name, x in _absmax_cases(_dt(dtype)).items():
        x = x.reshape(-1, x.shape[-1]).clone() if x.is_contiguous() else x
        clean_c, clean_r = x.float().abs().amax(0), x.float().abs().amax(1)
        r, c = x.shape[0] * 2 // 3, x.shape[1] * 2 // 3
        x[r, c] = float("nan")
        cols, rows = ops.absmax(x), ops.absmax(x, per_row=True)
        keep_c = torch.arange(x.shape[1], device="cuda") != c
        keep_r = torch.arange(x.shape[0], device="cuda") != r
        assert torch.isnan(cols[c]) and torch.equal(cols[keep_c], clean_c[keep_c]), name
        assert torch.isnan(rows[r]) and torch.equal(rows[keep_r], clean_r[keep_r]), name


# ------------------------------------------------------------------------------------ no fp32 copy
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_fp32_copy_of_the_activation_is_made(dtype):
    """A 32 Mi-element half tensor is 64 MB; its fp32 copy would be 128 MB.  The native path allocates a state, an output and
    a workspace of about 1 MB."""
    import torch
    from onnx_quantize_amd.calibration import MinMaxCalibrator
    from onnx_quantize_amd.hip import ops
    x = torch.ones(8192, 4096, dtype=_dt(dtype), device="cuda")
    x[4000, 77] = -5.0
    cal = MinMaxCalibrator()
    cal.collect("x", x)                                                # the warm call: workspaces exist from here on
    ops.absmax(x)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    cal.collect("x", x)
    cal.collect_many({"x": x, "y": x[:4096]})
    amax = ops.absmax(x)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert rise < x.numel() * x.element_size() // 4, rise
    assert cal.data["x"].min_val == -5.0 and cal.data["x"].max_val == 1.0 and amax[77] == 5.0 and amax[78] == 1.0


# ------------------------------------------------------------------------------------ the driver
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_driver_on_a_half_model_equals_a_stream_fed_the_upcasts(dtype):
    import torch
    from onnx_quantize_amd import calibration_driver as D
    from onnx_quantize_amd.calibration import MinMaxCalibrator
    from onnx_quantize_amd.config import QActivationArgs
    from onnx_quantize_amd.dtypes import QuantType
    torch.manual_seed(4)
    model = torch.nn.Sequential()
    model.add_module("fc1", torch.nn.Linear(40, 72))
    model.add_module("act", torch.nn.ReLU())
    model.add_module("fc2", torch.nn.Linear(72, 24))
    model = model.cuda().to(_dt(dtype))
    taps = {"X": ("fc1", "input"), "h1": ("fc1", "output"), "a1": ("fc2", "input"), "y": ("fc2", "output")}
    names = dict(input_names=["X", "a1"], output_names=["h1", "y"], absmax_names=["X", "a1"])
    data = (torch.randn(40, 7, 40) * 2).to(_dt(dtype))
    runner = D.TorchRunner(model, taps)
    seen = []

    def recording(feed):
        out = runner(feed)
        seen.append(out)
        return out

    native = D.run_calibration(recording, data, D.ActivationStream(calibrator=MinMaxCalibrator(0.8), **names), num_samples=40, batch_size=10)
    runner.close()
    assert native.batches == 4 and all(t.dtype == _dt(dtype) for b in seen for t in b.values())
    upcast = D.ActivationStream(calibrator=MinMaxCalibrator(0.8), **names)
    for b in seen:
        upcast.feed({n: t.float() for n, t in b.items()})
    in_args = QActivationArgs(dtype=QuantType.QUInt8, is_static=True)
    out_args = QActivationArgs(dtype=QuantType.QInt8, symmetric=True, is_static=True)
    for got, ref, want in ((native.input_qparams(in_args), upcast.input_qparams(in_args), {"X", "a1"}),
                           (native.output_qparams(out_args), upcast.output_qparams(out_args), {"h1", "y"})):
        assert got.keys() == ref.keys() == want
        for n in want:
            assert got[n][0].tobytes() == ref[n][0].tobytes() and got[n][1].tobytes() == ref[n][1].tobytes(), (n, got[n], ref[n])
    assert native.absmax.keys() == upcast.absmax.keys() == {"X", "a1"}
    for n in native.absmax:
        assert native.absmax[n].dtype == torch.float32 and torch.equal(native.absmax[n], upcast.absmax[n]), n
