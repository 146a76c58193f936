"""The AWQ / SmoothQuant searches on fp16 / bf16 weights in the half-precision extension of the C ABI (include/oq_hip_half.h, N2h):
the seven symbols are declared, bound and exported, the extension version stays 1, the workspace queries follow the formula the
header states, and hostile arguments are refused with the stated status -- without a GPU.

Every library call below is one the checks must REFUSE before any device work: the pointers are host memory standing in for
device memory and nothing may be launched on them.  The second half runs the model layer with the oracle as numeric provider:
`half_weights="native_calibrated"` takes the preprocessors in front of weight-only RTN and refuses the rest by name."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from half_model_helpers import half_model, upcasting_oracle

HEADER = os.path.join(ROOT, "include", "oq_hip_half.h")
NEW = {"oq_awq_half_workspace_bytes": 3, "oq_awq_stats_half_workspace_bytes": 2, "oq_awq_scale_search_h16": 20, "oq_awq_clip_search_h16": 18,
       "oq_awq_scale_search_stats_h16": 20, "oq_awq_clip_search_stats_h16": 17, "oq_smooth_quant_scale_h16": 13}
F16, BF16, UINT4, GROUP = 0, 1, 1, 2
HUGE = (1 << 62) + 12345


@pytest.fixture(scope="module")
def lib_path():
    from onnx_quantize_amd import _build
    return _build.build(verbose=False)


@pytest.fixture(scope="module")
def lib(lib_path):
    from onnx_quantize_amd.hip import _lib
    return _lib.load()


def test_the_prototypes_are_declared_bound_and_exported(lib_path):
    from onnx_quantize_amd.hip import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(oq_[a-z0-9_]+)\s*\(", text))
    raw = C.CDLL(lib_path)
    for name, nargs in NEW.items():
        assert name in declared, f"{name} is not declared in include/oq_hip_half.h"
        assert name in _lib.HALF_PROTOTYPES, f"{name} is not in _lib.HALF_PROTOTYPES"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert len(_lib.HALF_PROTOTYPES[name][1]) == nargs, name
        twin = name.replace("_h16", "_f32")
        if twin != name:                                                        # the twin's arguments plus `wtype`
            assert len(_lib.PROTOTYPES[twin][1]) == nargs - 1, name
    assert declared == set(_lib.HALF_PROTOTYPES)
    assert raw.oq_half_extension_version() == 1 == _lib.OQ_HALF_EXTENSION_VERSION
    assert _lib.OQ_ABI_VERSION == 2


# ------------------------------------------------------------------------------------ the workspace queries
def _extra(k, n):
    """R(K, N) of the header: 8 * N * (ceil(K / 64) + K / 257 + 1) rounded up to 256, + 256."""
    return -(-8 * n * (-(-k // 64) + k // 257 + 1) // 256) * 256 + 256


@pytest.mark.parametrize("shape", [(96, 256, 64), (1, 4, 1), (48, 1100, 256), (4096, 4096, 4096), (3 * 160, 160, 7)])
def test_workspace_queries_follow_the_header_inside_the_bounds(lib, shape):
    t, k, n = shape
    assert lib.oq_awq_workspace_bytes(t, k, n) > 0 and lib.oq_awq_stats_workspace_bytes(k, n) > 0
    assert lib.oq_awq_half_workspace_bytes(t, k, n) == lib.oq_awq_workspace_bytes(t, k, n) + _extra(k, n)
    assert lib.oq_awq_stats_half_workspace_bytes(k, n) == lib.oq_awq_stats_workspace_bytes(k, n) + _extra(k, n)
    # what R is for: the partial ranges of oq_rtn_quantize_h16 on any strategy and group of this shape fit
    for strategy, g in ((0, -1), (1, -1), (2, k), (2, -1)) + tuple((2, d) for d in (257, 300, 512) if k % d == 0):
        assert lib.oq_rtn_half_workspace_bytes(k, n, strategy, g) <= _extra(k, n) - 256, (strategy, g)


OUTSIDE = [("T=0", (0, 64, 8)), ("K=0", (16, 0, 8)), ("N=0", (16, 64, 0)), ("K=-1", (16, -1, 8)), ("K=65536", (16, 65536, 8)),
           ("K=2^62", (16, HUGE, 8)), ("N=2^62", (16, 64, HUGE)), ("T=2^62", (HUGE, 64, 8)), ("K*N>2^40", (16, 65535, 1 << 30))]


@pytest.mark.parametrize("case", OUTSIDE, ids=[c[0] for c in OUTSIDE])
def test_workspace_queries_return_zero_outside_the_bounds(lib, case):
    t, k, n = case[1]
    assert lib.oq_awq_half_workspace_bytes(t, k, n) == 0
    if not case[0].startswith("T="):
        assert lib.oq_awq_stats_half_workspace_bytes(k, n) == 0


# ------------------------------------------------------------------------------------ hostile arguments
ORDER = {
    "oq_awq_scale_search_h16": "X T K ldx W wtype N ldw qtype strategy g sym rr n_grid scales losses best ws ws_bytes stream",
    "oq_awq_clip_search_h16": "X T K ldx W wtype N ldw qtype strategy g sym rr losses best ws ws_bytes stream",
    "oq_awq_scale_search_stats_h16": "act G T K W wtype N ldw qtype strategy g sym rr n_grid scales losses best ws ws_bytes stream",
    "oq_awq_clip_search_stats_h16": "G T K W wtype N ldw qtype strategy g sym rr losses best ws ws_bytes stream",
    "oq_smooth_quant_scale_h16": "X T K ldx W wtype N ldw alpha scale ws ws_bytes stream",
}
AWQ = [n for n in ORDER if "awq" in n]
SCALE = [n for n in ORDER if "scale_search" in n]
ALL = list(ORDER)


@pytest.fixture(scope="module")
def host():
    buf = (C.c_char * (1 << 16))()
    base = C.addressof(buf)
    yield buf, base + (-base % 256)


def _args(name, ptr, **over):
    a = dict(X=ptr, T=16, K=64, ldx=64, act=ptr, G=ptr, W=ptr + 4096, wtype=F16, N=8, ldw=8, qtype=UINT4, strategy=GROUP, g=16, sym=0, rr=0,
             n_grid=20, scales=ptr + 8192, losses=ptr + 8192, best=ptr + 8192, scale=ptr + 8192, alpha=0.5, ws=ptr + 16384, ws_bytes=1 << 40,
             stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return [a[f] for f in ORDER[name].split()]


# (what is hostile, entry points, overrides, statuses allowed, a word of the message)
CASES = [
    ("wtype=2", ALL, dict(wtype=2), (-1,), "wtype"), ("wtype=-1", ALL, dict(wtype=-1), (-1,), "wtype"),
    ("W odd", ALL, "odd", (-1,), "2-byte aligned"), ("W null", ALL, dict(W=None), (-1,), "bad argument"),
    ("K=0", ALL, dict(K=0), (-1,), "bad argument"), ("N=-1", ALL, dict(N=-1), (-1,), "bad argument"), ("ldw<N", ALL, dict(ldw=7), (-1,), "bad argument"),
    ("N=2^62", ALL, dict(N=HUGE, ldw=HUGE), (-1,), "bad argument"),
    ("n_grid=0", SCALE, dict(n_grid=0), (-1,), "bad argument"), ("n_grid=65", SCALE, dict(n_grid=65), (-1,), "bad argument"),
    ("losses null", AWQ, dict(losses=None), (-1,), "bad argument"), ("best null", AWQ, dict(best=None), (-1,), "bad argument"),
    ("group=3", AWQ, dict(g=3), (-2,), "group_size"), ("group=24", AWQ, dict(g=24), (-2,), "group_size"),
    ("K=65536", AWQ, dict(K=65536, ldx=65536, g=128), (-2,), "K too large"), ("qtype int16", AWQ, dict(qtype=4), (-2, -1), "awq"),
    ("strategy=9", AWQ, dict(strategy=9), (-1,), "strategy"),
    ("workspace null", ALL, dict(ws=None), (-3,), "workspace"), ("workspace short", ALL, dict(ws_bytes=4096), (-3,), "workspace"),
    ("workspace misaligned", AWQ, "misaligned", (-3,), "workspace"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hostile_arguments_are_refused_on_the_host(lib, host, case):
    buf, ptr = host
    _, names, over, allowed, word = case
    for name in names:
        o = dict(W=ptr + 4097) if over == "odd" else dict(ws=ptr + 16384 + 64) if over == "misaligned" else over
        before = bytes(buf)
        st = getattr(lib, name)(*_args(name, ptr, **o))
        msg = lib.oq_last_error().decode()
        assert st in allowed, (name, st, msg)
        assert word in msg, (name, msg)
        assert bytes(buf) == before, name                     # nothing written on failure


# ------------------------------------------------------------------------------------ the model layer (oracle as numeric provider)
SEED = 3


def _case(seed=SEED):
    """tests/test_awq_half_file_gpu.py::case."""
    r = np.random.default_rng(seed)
    w = (r.standard_normal((256, 64)) * 0.05).astype(np.float16)
    x = r.standard_normal((128, 256)) * r.uniform(0.1, 4, 256)
    x[:, r.choice(256, 8, replace=False)] *= 30
    return w, x.astype(np.float16)


def _run(data, qc, **kw):
    import oq_oracle as O
    from onnx_model_helpers import OracleSearches, oracle_calibrate
    from onnx_quantize_amd.model_quantize import quantize_model
    return quantize_model(data, qc, weight_arrays=upcasting_oracle, quantize_bias=O.quantize_bias, calibrate=oracle_calibrate(),
                          searches=OracleSearches(), **kw)


def _qc(x, pre, algorithm=None):
    from onnx_quantize_amd import CalibrationParams, QConfig, QuantType, QWeightArgs
    weights = QWeightArgs(dtype=QuantType.QUInt4, group_size=32, strategy="group", **({"algorithm": algorithm} if algorithm else {}))
    return QConfig(weights=weights, preprocessors=[pre], calibration_data=x, calibration_params=CalibrationParams(num_samples=128, batch_size=128))


def test_the_seed_of_the_file_tests_is_a_test():
    """What makes the inputs of tests/test_awq_half_file_gpu.py a test, from the oracle on the upcast inputs: the best candidate
    lies inside the grid and wins clearly, and the reciprocal of every scale is a normal fp16."""
    import oq_oracle as O
    w, x = _case()
    s, losses = O.awq_scale_search(x.astype(np.float32), w.astype(np.float32), "uint4", "group", 32)
    best = int(np.argmin(losses))
    r16 = (np.float32(1) / s).astype(np.float16)
    print(f"best candidate {best}, loss {losses[best] / losses[0]:.3f} of candidate 0's, s in {s.min():.3f} .. {s.max():.3f}")
    assert 2 <= best <= 17 and losses[best] < 0.5 * losses[0]
    assert np.isfinite(r16).all() and (np.abs(r16) >= np.finfo(np.float16).tiny).all()
    s_eff = np.float32(1) / r16.astype(np.float32)
    assert 2.0 ** -13 < np.abs(s_eff / s - 1).max() <= 2.0 ** -11       # the rounding the s_eff rule is about is there


@pytest.mark.parametrize("pre", ["awq", "awq_clip", "smooth_quant"])
def test_native_calibrated_takes_the_preprocessors(pre):
    import oq_oracle as O
    from onnx_quantize_amd import AwqConfig, SmoothQuantConfig
    from onnx_quantize_amd.onnx_proto import DataType, serialize, tensor_to_numpy

    w, x = _case()
    cfg = {"awq": AwqConfig(clip_search=False), "awq_clip": AwqConfig(clip_search=True), "smooth_quant": SmoothQuantConfig(alpha=0.5)}[pre]
    out = _run(serialize(half_model([w])), _qc(x, cfg), half_weights="native_calibrated")
    assert [n.op_type for n in out.graph.node] == ["Mul", "MatMulNBits"]
    mul, node = out.graph.node
    inits = {t.name: t for t in out.graph.initializer}
    assert inits[mul.input[1]].data_type == DataType.FLOAT16 and inits[node.input[2]].data_type == DataType.FLOAT16
    assert inits[node.input[1]].data_type == DataType.UINT8
    w32, x32 = w.astype(np.float32), x.astype(np.float32)
    s = O.smooth_quant_scale(x32, w32, 0.5) if pre == "smooth_quant" else O.awq_scale_search(x32, w32, "uint4", "group", 32)[0]
    r16 = (np.float32(1) / np.asarray(s, dtype=np.float32)).astype(np.float16)
    assert tensor_to_numpy(inits[mul.input[1]]).tobytes() == r16.tobytes()
    # the weight's side took s_eff = 1 / fp32(r16), not the searched s: the stored integers are those of s_eff[:, None] * W
    s_eff = np.float32(1) / r16.astype(np.float32)
    w_eff = s_eff.reshape(-1, 1) * w32
    ratio = 1.0
    if pre == "awq_clip":
        ratio, _ = O.awq_clip_search(x32 / s_eff.reshape(1, -1), w_eff, "uint4", "group", 32)
    q, sc, z = O.seam_arrays(w_eff, "rtn", "uint4", "group", 32, False, False, ratio, False, x=None, nbits=True)
    assert tensor_to_numpy(inits[node.input[1]]).tobytes() == np.asarray(q).tobytes()
    assert tensor_to_numpy(inits[node.input[2]]).tobytes() == np.asarray(sc, dtype=np.float32).astype(np.float16).tobytes()


def test_consumers_of_one_half_value_share_one_upcast_input():
    """Two MatMuls that read X: the second searches on the input the first one divided (awq.py:191, in place)."""
    import oq_oracle as O
    from onnx_quantize_amd import SmoothQuantConfig
    from onnx_quantize_amd.onnx_proto import DataType, Message, make_node, make_value_info, numpy_to_tensor, serialize, tensor_to_numpy

    w, x = _case()
    w2 = (np.random.default_rng(SEED + 1).standard_normal((256, 32)) * 0.05).astype(np.float16)
    g = Message("GraphProto", name="fan", node=[make_node("MatMul", ["X", "W0"], ["Y0"], name="fc0"), make_node("MatMul", ["X", "W1"], ["Y1"], name="fc1")],
                initializer=[numpy_to_tensor("W0", w), numpy_to_tensor("W1", w2)], input=[make_value_info("X", DataType.FLOAT16, ["N", 256])],
                output=[make_value_info("Y0", DataType.FLOAT16, ["N", 64]), make_value_info("Y1", DataType.FLOAT16, ["N", 32])])
    model = Message("ModelProto", ir_version=10, graph=g, opset_import=[Message("OperatorSetIdProto", domain="", version=21)])
    out = _run(serialize(model), _qc(x, SmoothQuantConfig(alpha=0.5)), half_weights="native_calibrated")
    inits = {t.name: tensor_to_numpy(t) for t in out.graph.initializer}
    x32 = x.astype(np.float32)
    s0 = np.asarray(O.smooth_quant_scale(x32, w.astype(np.float32), 0.5), dtype=np.float32)
    r0 = (np.float32(1) / s0).astype(np.float16)
    assert inits["Y0_scale"].tobytes() == r0.tobytes()
    divided = x32 / (np.float32(1) / r0.astype(np.float32)).reshape(1, -1)
    s1 = np.asarray(O.smooth_quant_scale(divided, w2.astype(np.float32), 0.5), dtype=np.float32)
    assert inits["Y1_scale"].tobytes() == (np.float32(1) / s1).astype(np.float16).tobytes()


def test_what_stays_refused_is_refused_by_name():
    from onnx_quantize_amd import AwqConfig, GPTQConfig, SmoothQuantConfig
    from onnx_quantize_amd.model_quantize import apply_pre_passes
    from onnx_quantize_amd.onnx_proto import serialize
    from onnx_model_helpers import OracleSearches, oracle_calibrate

    w, x = _case()
    data = serialize(half_model([w]))
    for pre in (AwqConfig(), SmoothQuantConfig()):
        with pytest.raises(NotImplementedError, match="preprocessors"):
            _run(data, _qc(x, pre), half_weights="native")
    with pytest.raises(NotImplementedError, match="gptq"):
        _run(data, _qc(x, AwqConfig(), algorithm=GPTQConfig()), half_weights="native_calibrated")
    with pytest.raises(NotImplementedError, match="post_calibration"):
        apply_pre_passes(data, _qc(x, AwqConfig()), device="cpu", calibrate=oracle_calibrate(), searches=OracleSearches(), post_calibration="always",
                         half_weights="native_calibrated")
    with pytest.raises(NotImplementedError, match="half precision"):
        _run(data, _qc(x, AwqConfig()))                                         # half_weights="error", the default


def test_a_reciprocal_outside_the_normal_fp16_range_names_node_and_channel():
    from onnx_quantize_amd import SmoothQuantConfig
    from onnx_quantize_amd.model_quantize import _half_mul_scale
    from onnx_quantize_amd.onnx_proto import serialize

    w, x = _case()
    x = x.copy()
    x[:, 5] = np.float16(2.0 ** -24)
    with pytest.raises(ValueError, match=r"node 'fc0'.*channel 5"):
        _run(serialize(half_model([w])), _qc(x, SmoothQuantConfig(alpha=1.0)), half_weights="native_calibrated")
    ok = np.array([1.0, 0.25, 4.0], dtype=np.float32)
    r16, s_eff = _half_mul_scale(ok, "n")
    assert r16.dtype == np.float16 and s_eff.dtype == np.float32 and np.array_equal(s_eff, ok)
    for bad in (1e-5, 1e5, np.inf, np.nan, 0.0):                              # 1 / s: inf, subnormal, zero, NaN, inf
        with pytest.raises(ValueError, match="channel 1"):
            _half_mul_scale(np.array([1.0, bad, 2.0], dtype=np.float32), "n")
