"""The half-precision extension of the C ABI (include/oq_hip_half.h): declared, bound and exported as one set, plain C99, and
its argument checks answer without a GPU.  oq_hip.h and its pins (tests/test_library_abi.py) are untouched: ABI version 2.

Every call of the sweep below is one the checks must REFUSE before any device call, so this file is safe on a box with a GPU
too: the pointers are host memory standing in for device memory and nothing may be launched on them."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "oq_hip_half.h")
BASE_HEADER = os.path.join(ROOT, "include", "oq_hip.h")


def declared_symbols(path):
    """The regular expression of tests/test_library_abi.py."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(oq_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib_path():
    from onnx_quantize_amd import _build
    return _build.build(verbose=False)


@pytest.fixture(scope="module")
def lib(lib_path):
    from onnx_quantize_amd.hip import _lib
    return _lib.load()


def test_half_header_matches_ctypes_prototypes_and_the_library_exports_them(lib_path):
    from onnx_quantize_amd.hip import _lib
    assert declared_symbols(HEADER) == sorted(_lib.HALF_PROTOTYPES)
    assert _lib.WTYPE_CODE == {"float16": 0, "bfloat16": 1}
    raw = C.CDLL(lib_path)
    for name in declared_symbols(HEADER):
        assert hasattr(raw, name), f"{name} is declared in include/oq_hip_half.h but not exported"
    assert raw.oq_half_extension_version() == 1


def test_half_header_is_plain_c99(tmp_path):
    src = tmp_path / "half_header.c"
    src.write_text('#include "oq_hip_half.h"\n'
                   "typedef void (*fn)(void);\n"
                   "fn taken[] = {(fn)oq_half_extension_version, (fn)oq_rtn_half_workspace_bytes, (fn)oq_rtn_quantize_h16};\n"
                   "int codes[] = {OQ_W_F16, OQ_W_BF16, OQ_HALF_EXTENSION_VERSION, OQ_LAYOUT_NBITS};\n")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                         str(tmp_path / "half_header.o")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr


def test_the_base_abi_is_unchanged(lib):
    from onnx_quantize_amd.hip import _lib
    assert lib.oq_abi_version() == 2 == _lib.OQ_ABI_VERSION
    assert declared_symbols(BASE_HEADER) == sorted(_lib.PROTOTYPES)
    assert not set(_lib.PROTOTYPES) & set(_lib.HALF_PROTOTYPES)


# ------------------------------------------------------------------------------------ hostile arguments
F16, GROUP, CHANNEL, UINT4, KN, NBITS, PACKED4 = 0, 2, 1, 1, 0, 1, 2


@pytest.fixture(scope="module")
def host_ptr():
    buf = (C.c_char * (1 << 16))()
    base = C.addressof(buf)
    yield buf, base + (-base % 16)


def quantize_args(ptr, **over):
    a = dict(W=ptr, wtype=F16, K=256, N=64, ldw=64, qtype=UINT4, strategy=GROUP, group_size=128, symmetric=0, reduce_range=0,
             clip_ratio=1.0, q_out=ptr, scale_out=ptr, zp_out=ptr, layout=KN, workspace=None, workspace_bytes=0, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


HUGE = (1 << 62) + 12345
QUANTIZE_CASES = [
    # (what is hostile, overrides, statuses allowed, a word of the message that names the argument)
    ("K=0", dict(K=0), (-1,), "K=0"), ("K=-1", dict(K=-1), (-1,), "K=-1"), ("K=2^62", dict(K=HUGE), (-1, -2), "K="),
    ("N=0", dict(N=0), (-1,), "N=0"), ("N=-1", dict(N=-1), (-1,), "N=-1"), ("N=2^62", dict(N=HUGE, ldw=HUGE), (-1, -2), "N="),
    ("ldw=2^62", dict(ldw=HUGE), (-1, -2), "ldw="), ("ldw<N", dict(ldw=63), (-1,), "ldw=63"),
    ("all huge", dict(K=HUGE, N=HUGE, ldw=HUGE, group_size=HUGE, workspace_bytes=1 << 62), (-1, -2), "K="),
    ("all 2^41", dict(K=1 << 41, N=1 << 41, ldw=1 << 41, group_size=1 << 41), (-1, -2), "K="),
    ("2^31 x 2^31", dict(K=(1 << 31) - 1, N=(1 << 31) - 1, ldw=(1 << 31) - 1), (-2,), "too large"),
    ("wtype", dict(wtype=2), (-1,), "wtype"), ("wtype<0", dict(wtype=-1), (-1,), "wtype"),
    ("qtype", dict(qtype=99), (-1,), "quantization type"), ("qtype 32 bit", dict(qtype=4), (-2,), "32-bit"),
    ("strategy", dict(strategy=9), (-1,), "strategy"), ("layout", dict(layout=9), (-1,), "layout"),
    ("layout packed4", dict(layout=PACKED4), (-2,), "KN_PACKED4"),
    ("group_size=0", dict(group_size=0), (-1,), "group_size"), ("group_size=-5", dict(group_size=-5), (-1,), "group_size"),
    ("straddling groups", dict(group_size=96), (-2,), "group_size 96"),
    ("clip 0", dict(clip_ratio=0.0), (-1,), "clip_ratio"), ("clip 1.5", dict(clip_ratio=1.5), (-1,), "clip_ratio"),
    ("clip nan", dict(clip_ratio=float("nan")), (-1,), "clip_ratio"),
    ("null W", dict(W=None), (-1,), "null W"), ("null scale", dict(scale_out=None), (-1,), "scale_out"),
    ("null zp", dict(zp_out=None), (-1,), "zp_out"), ("null q, blob", dict(q_out=None, layout=NBITS), (-2,), "q_out"),
    ("blob, channel", dict(layout=NBITS, strategy=CHANNEL), (-2,), "NBITS"),
    ("blob, group of 8", dict(layout=NBITS, group_size=8), (-2,), "group_size % 16"),
    ("no workspace", dict(strategy=CHANNEL), (-3,), "workspace"),
]


@pytest.mark.parametrize("case", QUANTIZE_CASES, ids=[c[0] for c in QUANTIZE_CASES])
def test_quantize_h16_refuses_hostile_arguments(lib, host_ptr, case):
    _, ptr = host_ptr
    _, over, allowed, word = case
    st = lib.oq_rtn_quantize_h16(*quantize_args(ptr, **over))
    msg = lib.oq_last_error().decode()
    assert st in allowed, (st, msg)
    assert word in msg, msg


def test_quantize_h16_refuses_a_short_workspace_and_a_misaligned_blob(lib, host_ptr):
    _, ptr = host_ptr
    need = lib.oq_rtn_half_workspace_bytes(256, 64, CHANNEL, -1)
    assert need == 2 * 4 * 64 * 4                     # min and max of four 64-row chunks of every column, fp32
    assert lib.oq_rtn_half_workspace_bytes(256, 64, GROUP, 128) == 0
    st = lib.oq_rtn_quantize_h16(*quantize_args(ptr, strategy=CHANNEL, workspace=ptr, workspace_bytes=need - 1))
    assert st == -3 and str(need) in lib.oq_last_error().decode()
    for off in (1, 4, 8):
        st = lib.oq_rtn_quantize_h16(*quantize_args(ptr, layout=NBITS, q_out=ptr + off))
        assert st == -2 and "16-byte aligned q_out" in lib.oq_last_error().decode()
    st = lib.oq_rtn_quantize_h16(*quantize_args(ptr, W=ptr + 1))
    assert st == -1 and "2-byte aligned" in lib.oq_last_error().decode()


WORKSPACE_CASES = [("K=0", (0, 64, GROUP, 128), "K=0"), ("K=-1", (-1, 64, GROUP, 128), "K=-1"), ("K=2^62", (HUGE, 64, GROUP, 128), "K="),
                   ("N=0", (256, 0, GROUP, 128), "N=0"), ("N=-1", (256, -1, CHANNEL, -1), "N=-1"), ("N=2^62", (256, HUGE, CHANNEL, -1), "N="),
                   ("all huge", (HUGE, HUGE, GROUP, HUGE), "K="), ("strategy", (256, 64, 9, 128), "strategy"),
                   ("group_size=0", (256, 64, GROUP, 0), "group_size"), ("straddling", (256, 64, GROUP, 96), "straddle")]


@pytest.mark.parametrize("case", WORKSPACE_CASES, ids=[c[0] for c in WORKSPACE_CASES])
def test_half_workspace_query_refuses_hostile_arguments(lib, case):
    _, args, word = case
    assert lib.oq_rtn_half_workspace_bytes(*args) == 0
    assert word in lib.oq_last_error().decode()


# ------------------------------------------------------------------------------------ the file path, opt-in (oracle as numeric provider)
from half_model_helpers import half_model, upcasting_oracle  # noqa: E402


def test_native_half_weights_emit_matmul_nbits_with_float16_scales():
    import numpy as np
    import oq_oracle as O
    from onnx_quantize_amd import QConfig, QuantType, QWeightArgs
    from onnx_quantize_amd.model_quantize import quantize_model
    from onnx_quantize_amd.onnx_proto import DataType, check_model, parse_model, serialize, tensor_to_numpy

    w16 = np.random.default_rng(0).standard_normal((64, 8)).astype(np.float16)
    qc = lambda: QConfig(weights=QWeightArgs(dtype=QuantType.QUInt4, group_size=32, strategy="group"))      # noqa: E731
    half = quantize_model(serialize(half_model([w16])), qc(), weight_arrays=upcasting_oracle, quantize_bias=O.quantize_bias, half_weights="native")
    full = quantize_model(serialize(half_model([w16.astype(np.float32)])), qc(), weight_arrays=upcasting_oracle, quantize_bias=O.quantize_bias)
    assert [n.op_type for n in half.graph.node] == ["MatMulNBits"] == [n.op_type for n in full.graph.node]
    ih = {t.name: t for t in half.graph.initializer}
    if_ = {t.name: t for t in full.graph.initializer}
    node = half.graph.node[0]
    b, s, z = node.input[1], node.input[2], node.input[3]
    assert tensor_to_numpy(ih[b]).tobytes() == tensor_to_numpy(if_[b]).tobytes()
    assert tensor_to_numpy(ih[z]).tobytes() == tensor_to_numpy(if_[z]).tobytes()
    assert ih[s].data_type == DataType.FLOAT16 and if_[s].data_type == DataType.FLOAT
    scales32 = tensor_to_numpy(if_[s])
    assert scales32.dtype == np.float32
    assert tensor_to_numpy(ih[s]).tobytes() == np.float16(scales32).tobytes()
    _, es, _ = O.rtn_quantize(w16.astype(np.float32), "uint4", "group", 32)
    assert scales32.tobytes() == np.asarray(es, np.float32).tobytes()
    check_model(half)
    check_model(parse_model(serialize(half)))


def test_native_half_weights_refuse_what_is_unsupported_by_name():
    import numpy as np
    import oq_oracle as O
    from onnx_model_helpers import oracle_calibrate
    from onnx_quantize_amd import GPTQConfig, HqqConfig, QActivationArgs, QConfig, QuantType, QWeightArgs
    from onnx_quantize_amd.model_quantize import quantize_model
    from onnx_quantize_amd.onnx_proto import serialize

    w16 = np.random.default_rng(1).standard_normal((64, 8)).astype(np.float16)
    data = serialize(half_model([w16]))
    run = lambda qc, **kw: quantize_model(data, qc, weight_arrays=upcasting_oracle, quantize_bias=O.quantize_bias,      # noqa: E731
                                          calibrate=oracle_calibrate(), **kw)
    with pytest.raises(NotImplementedError, match="float32"):                              # the default stays
        run(QConfig(weights=QWeightArgs(dtype=QuantType.QUInt4, group_size=32, strategy="group")))
    with pytest.raises(NotImplementedError, match="MatMulNBits"):                          # a QDQ rule: int8 per channel
        run(QConfig(weights=QWeightArgs(dtype=QuantType.QInt8, strategy="channel")), half_weights="native")
    with pytest.raises(NotImplementedError, match="calibrat"):                             # GPTQ needs calibration
        run(QConfig(weights=QWeightArgs(dtype=QuantType.QUInt4, group_size=32, strategy="group", algorithm=GPTQConfig())), half_weights="native")
    with pytest.raises(NotImplementedError, match="hqq"):                                  # HQQ: float zero points next to the scales
        run(QConfig(weights=QWeightArgs(dtype=QuantType.QUInt4, group_size=32, strategy="group", algorithm=HqqConfig())), half_weights="native")
    with pytest.raises(NotImplementedError, match="activation"):                           # static activations
        run(QConfig(weights=QWeightArgs(dtype=QuantType.QInt8), input_activations=QActivationArgs(is_static=True)), half_weights="native")
    with pytest.raises(ValueError, match="half_weights"):
        run(QConfig(weights=QWeightArgs()), half_weights="maybe")
