"""The GPTQ Hessian of fp16 / bf16 activations in the half-precision extension of the C ABI (include/oq_hip_half.h):
declared, bound and exported, its argument checks answer without a GPU, and the file path's opt-in value
`half_weights="native_calibrated"` accepts and refuses what it says -- with the oracle as numeric provider, so nothing here
needs a device.

Every library call below is one the checks must REFUSE before any device work: the pointers are host memory standing in for
device memory and nothing may be launched on them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from half_model_helpers import half_model, upcasting_oracle

HEADER = os.path.join(ROOT, "include", "oq_hip_half.h")
NEW = ("oq_hessian_half_workspace_bytes", "oq_hessian_accumulate_h16")


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
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/oq_hip_half.h"
        assert name in _lib.HALF_PROTOTYPES, f"{name} is not in _lib.HALF_PROTOTYPES"
        assert hasattr(raw, name), f"{name} is not exported by the library"
    assert len(_lib.HALF_PROTOTYPES["oq_hessian_accumulate_h16"][1]) == 11
    assert len(_lib.HALF_PROTOTYPES["oq_hessian_half_workspace_bytes"][1]) == 2
    assert raw.oq_half_extension_version() == 1 == _lib.OQ_HALF_EXTENSION_VERSION        # additions only: the pin stays


# ------------------------------------------------------------------------------------ hostile arguments
F16, BF16 = 0, 1
HUGE = (1 << 62) + 12345


@pytest.fixture(scope="module")
def host_ptr():
    buf = (C.c_char * (1 << 16))()
    base = C.addressof(buf)
    yield buf, base + (-base % 16)


def accumulate_args(ptr, **over):
    a = dict(X=ptr, xtype=F16, T=64, K=32, ldx=32, n_seen=0, n_add=4, H=ptr, workspace=ptr, workspace_bytes=1 << 16, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


ACCUMULATE_CASES = [
    # (what is hostile, overrides, statuses allowed, a word of the message)
    ("null X", dict(X=None), (-1,), "null"), ("null H", dict(H=None), (-1,), "null"),
    ("odd X", dict(X="odd"), (-1,), "2-byte aligned"),
    ("xtype=7", dict(xtype=7), (-1,), "xtype"), ("xtype=-1", dict(xtype=-1), (-1,), "xtype"),
    ("T=0", dict(T=0), (-1,), "T=0"), ("T=-1", dict(T=-1), (-1,), "T=-1"), ("T=2^62", dict(T=HUGE), (-1, -2), "T="),
    ("K=0", dict(K=0), (-1,), "K=0"), ("K=-1", dict(K=-1), (-1,), "K=-1"), ("K=2^62", dict(K=HUGE, ldx=HUGE), (-1, -2), "K="),
    ("ldx<K", dict(ldx=31), (-1,), "ldx=31"), ("ldx=2^62", dict(ldx=HUGE), (-1, -2), "ldx="),
    ("K>2^17", dict(K=(1 << 17) + 1, ldx=(1 << 17) + 1), (-2,), "too large"),
    ("T*K>2^40", dict(T=1 << 24, K=1 << 17, ldx=1 << 17), (-2,), "too large"),
    ("T*ldx>2^40", dict(T=1 << 30, K=32, ldx=1 << 11), (-2,), "too large"),
    ("all huge", dict(T=HUGE, K=HUGE, ldx=HUGE, n_add=HUGE, workspace_bytes=1 << 62), (-1, -2), "T="),
    ("n_add=0", dict(n_add=0), (-1,), "sample counts"), ("n_seen=-1", dict(n_seen=-1), (-1,), "sample counts"),
    ("n_add=2^62", dict(n_add=HUGE), (-1,), "sample counts"),
    ("null workspace", dict(workspace=None), (-3,), "workspace"), ("short workspace", dict(workspace_bytes=64), (-3,), "workspace"),
]


@pytest.mark.parametrize("case", ACCUMULATE_CASES, ids=[c[0] for c in ACCUMULATE_CASES])
def test_accumulate_h16_refuses_hostile_arguments(lib, host_ptr, case):
    buf, ptr = host_ptr
    _, over, allowed, word = case
    over = {k: (ptr + 1 if v == "odd" else v) for k, v in over.items()}
    before = bytes(buf)
    st = lib.oq_hessian_accumulate_h16(*accumulate_args(ptr, **over))
    msg = lib.oq_last_error().decode()
    assert st in allowed, (st, msg)
    assert word in msg, msg
    assert bytes(buf) == before                                   # nothing written on failure


WORKSPACE_CASES = [("T=0", (0, 32)), ("T=-1", (-1, 32)), ("T=2^62", (HUGE, 32)), ("K=0", (64, 0)), ("K=-1", (64, -1)), ("K=2^62", (64, HUGE)),
                   ("K>2^17", (64, (1 << 17) + 1)), ("T*K>2^40", (1 << 24, 1 << 17)), ("all huge", (HUGE, HUGE))]


@pytest.mark.parametrize("case", WORKSPACE_CASES, ids=[c[0] for c in WORKSPACE_CASES])
def test_half_workspace_query_returns_zero_outside_the_bounds(lib, case):
    assert lib.oq_hessian_half_workspace_bytes(*case[1]) == 0


def test_half_workspace_query_inside_the_bounds(lib):
    # the packed operand: T padded to 32 rows x K padded to 256 columns x 2 bytes; then 16 slabs of K x K floats; 512 of slack
    assert lib.oq_hessian_half_workspace_bytes(64, 32) == 64 * 256 * 2 + 16 * 32 * 32 * 4 + 512
    assert lib.oq_hessian_half_workspace_bytes(33, 257) == 64 * 512 * 2 + 16 * 257 * 257 * 4 + 512


# ------------------------------------------------------------------------------------ the file path's option (oracle as numeric provider)
def _run(data, qc, **kw):
    import oq_oracle as O
    from onnx_model_helpers import oracle_calibrate
    from onnx_quantize_amd.model_quantize import quantize_model
    return quantize_model(data, qc, weight_arrays=upcasting_oracle, quantize_bias=O.quantize_bias, calibrate=oracle_calibrate(), **kw)


def test_native_calibrated_is_an_accepted_value_and_native_keeps_refusing_gptq():
    from onnx_quantize_amd import GPTQConfig, QConfig, QuantType, QWeightArgs
    from onnx_quantize_amd.model_quantize import HALF_WEIGHTS
    from onnx_quantize_amd.onnx_proto import DataType, serialize

    assert HALF_WEIGHTS == ("error", "native", "native_calibrated")
    w16 = np.random.default_rng(2).standard_normal((64, 8)).astype(np.float16)
    data = serialize(half_model([w16]))
    rtn = lambda: QConfig(weights=QWeightArgs(dtype=QuantType.QUInt4, group_size=32, strategy="group"))      # noqa: E731
    out = _run(data, rtn(), half_weights="native_calibrated")                    # weight-only RTN: what "native" gives
    ref = _run(data, rtn(), half_weights="native")
    assert [n.op_type for n in out.graph.node] == ["MatMulNBits"]
    assert serialize(out) == serialize(ref)
    scale = {t.name: t for t in out.graph.initializer}[out.graph.node[0].input[2]]
    assert scale.data_type == DataType.FLOAT16
    gptq = QConfig(weights=QWeightArgs(dtype=QuantType.QUInt4, group_size=32, strategy="group", algorithm=GPTQConfig()))
    with pytest.raises(NotImplementedError, match="calibrat"):
        _run(data, gptq, half_weights="native")
    with pytest.raises(ValueError, match="half_weights"):
        _run(data, rtn(), half_weights="calibrated")


def test_native_calibrated_refuses_what_is_unsupported_by_name():
    from onnx_quantize_amd import HqqConfig, QActivationArgs, QConfig, QuantType, QWeightArgs
    from onnx_quantize_amd.onnx_proto import DataType, serialize

    w16 = np.random.default_rng(3).standard_normal((64, 8)).astype(np.float16)
    data = serialize(half_model([w16]))
    with pytest.raises(NotImplementedError, match="hqq"):
        _run(data, QConfig(weights=QWeightArgs(dtype=QuantType.QUInt4, group_size=32, strategy="group", algorithm=HqqConfig())),
             half_weights="native_calibrated")
    with pytest.raises(NotImplementedError, match="activation"):
        _run(data, QConfig(weights=QWeightArgs(dtype=QuantType.QInt8), input_activations=QActivationArgs(is_static=True)),
             half_weights="native_calibrated")
    bf16 = half_model([w16])
    bf16.graph.initializer[0].data_type = DataType.BFLOAT16                     # the same 2-byte payload under the other type
    with pytest.raises(NotImplementedError, match="BFLOAT16"):
        _run(serialize(bf16), QConfig(weights=QWeightArgs(dtype=QuantType.QUInt4, group_size=32, strategy="group")), half_weights="native_calibrated")
