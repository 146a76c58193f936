"""The decode extension of the 8-bit QDQ function route (include/oq_hip_qdq_function_decode.h): declared, bound and exported as one
set with the argument lists of oq_hip_qdq_function.h, plain C99, its workspace query the header's sum on the host (0 with a message
for what the route refuses), and the two `qdq=` values that reach it accepted on any device."""
import ctypes as C
import os
import subprocess

import pytest
from conftest import ROOT
from test_qdq_function_abi import DYNAMIC, NONE, STATIC, declared_symbols, lib, lib_path, r256      # noqa: F401 -- its fixtures

HEADER = os.path.join(ROOT, "include", "oq_hip_qdq_function_decode.h")
MAX_K = 33025


def plan(M, K, N):      # include/oq_hip_qdq_function_decode.h, `plan`: (slice, splits)
    want = -(-(512 if M <= 4 else 256) // -(-N // 128))
    slice_ = min(2048, -(-(-(-K // want)) // 64) * 64)
    return slice_, -(-K // slice_)


def workspace(M, K, N, x_mode, out_mode):      # ... `workspace`: S + P + PX + PO
    blocks, splits = -(-N // 128), plan(M, K, N)[1]
    total = r256(splits * M * N * 4) if splits > 1 else 0
    if x_mode == DYNAMIC:
        total += r256(12) + r256(8 * -(-M // 4))
    if out_mode == DYNAMIC:
        total += r256(8 * (blocks if splits == 1 else -(-M * N // 256)))
    return total


def test_the_prototypes_are_declared_bound_and_exported(lib_path):
    from onnx_quantize_amd import _build
    from onnx_quantize_amd.hip import _lib, ops
    mine = _lib.QDQ_FUNCTION_DECODE_PROTOTYPES
    assert declared_symbols(HEADER) == sorted(mine) == ["oq_qdq_function_decode", "oq_qdq_function_decode_extension_version",
                                                        "oq_qdq_function_decode_workspace_bytes"]
    assert mine["oq_qdq_function_decode"] == _lib.QDQ_FUNCTION_PROTOTYPES["oq_qdq_function"]
    others = [p for p, *_ in _lib.EXTENSIONS if p is not mine]
    assert len(others) == len(_lib.EXTENSIONS) - 1 and not any(set(mine) & set(p) for p in others)
    raw = C.CDLL(lib_path)
    assert all(hasattr(raw, name) for name in mine)
    assert raw.oq_qdq_function_decode_extension_version() == 1 == _lib.OQ_QDQ_FUNCTION_DECODE_EXTENSION_VERSION
    assert raw.oq_abi_version() == 2 and raw.oq_qdq_function_extension_version() == 1      # additions only
    assert ops.QDQ_FUNCTION_DECODE_MAX_ROWS == 16
    assert _build.flags_for("qdq_function_decode.hip") == _build.flags_for("qdq_function.hip")      # one epilogue, one set of flags


def test_the_header_is_plain_c99(tmp_path):
    src = tmp_path / "header.c"
    src.write_text('#include "oq_hip_qdq_function_decode.h"\ntypedef void (*fn)(void);\n'
                   "fn taken[] = {(fn)oq_qdq_function_decode_extension_version, (fn)oq_qdq_function_decode_workspace_bytes, (fn)oq_qdq_function_decode};\n"
                   "int codes[] = {OQ_QDQ_FUNCTION_DECODE_EXTENSION_VERSION, OQ_QDQ_DYNAMIC, OQ_ERR_UNSUPPORTED};\n")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "header.o")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr


def test_the_workspace_is_the_headers_sum_and_zero_out_of_bounds(lib):
    query = lib.oq_qdq_function_decode_workspace_bytes
    assert query(16, 64, 260, STATIC, NONE) == 0                                      # one slice, nothing dynamic: no workspace
    assert query(16, 64, 260, DYNAMIC, DYNAMIC) == 256 + 256 + 256                   # P, PX (4 pairs), PO (3 column blocks)
    assert query(16, 4096, 11008, STATIC, NONE) == 3 * 16 * 11008 * 4                 # 86 column blocks want 3 slices: 1408, 1408, 1280
    assert query(1, 4096, 11008, STATIC, NONE) == 6 * 11008 * 4                       # up to 4 rows: 6 slices of 704
    for request_ in [(M, K, N, x, o) for M in (1, 4, 5, 16) for K, N in ((1, 1), (65, 128), (330, 16385), (11008, 4096), (MAX_K, 1))
                     for x, o in ((STATIC, NONE), (STATIC, DYNAMIC), (DYNAMIC, STATIC), (DYNAMIC, DYNAMIC))]:
        assert query(*request_) == workspace(*request_), request_
    for request_, words in (((17, 64, 8, STATIC, NONE), "M <= 16"), ((4, MAX_K + 1, 8, STATIC, NONE), "K <= 33025"), ((4, 64, 8, NONE, NONE), "x_mode=0")):
        assert query(*request_) == 0 and words in lib.oq_last_error().decode(), request_


@pytest.mark.parametrize("mode", ["fused+integer+decode", "fused+integer+decode+packed4"])
def test_the_modes_are_accepted_and_read_torch_on_the_host(mode):
    from onnx_quantize_amd import runner_routes as R
    from onnx_quantize_amd.graph_runner import GraphRunner
    from test_qdq_function_decode_runner_gpu import two_layers
    product, function = R.QDQ_MODES[mode]
    assert "integer_decode" in function and product == R.QDQ_MODES[mode.replace("+decode", "", 1)][0]
    runner = GraphRunner(two_layers(), device="cpu", qdq=mode)
    assert runner.qdq == "torch" and runner.qdq_function_calls == {"integer": 0, "body": 0} and runner.qdq_calls == {"fused": 0, "torch": 0}
    with pytest.raises(ValueError, match="qdq must be"):
        GraphRunner(two_layers(), device="cpu", qdq="fused+integer+packed4s")
