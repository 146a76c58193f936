"""The packed-nibble extension of the C ABI (include/oq_hip_qdq_packed4.h): declared, bound and exported as one set, plain C99, its
workspace query that of oq_qdq_matmul.  oq_hip_qdq.h keeps refusing the 4-bit type codes (test_qdq_matmul_abi.py)."""
import ctypes as C
import os
import subprocess

import pytest
from conftest import ROOT
from test_qdq_matmul_abi import BF16, F16, F32, SHAPES, declared_symbols, lib, lib_path      # noqa: F401 -- its fixtures

HEADER = os.path.join(ROOT, "include", "oq_hip_qdq_packed4.h")
INT4, UINT4 = 0, 1


def test_the_prototypes_are_declared_bound_and_exported(lib):
    from onnx_quantize_amd import _build
    from onnx_quantize_amd.hip import _lib
    assert declared_symbols(HEADER) == sorted(_lib.QDQ_PACKED4_PROTOTYPES)
    assert _lib.QDQ_PACKED4_PROTOTYPES["oq_qdq_matmul_packed4"] == _lib.QDQ_PROTOTYPES["oq_qdq_matmul"]      # one argument list
    raw = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, name) for name in _lib.QDQ_PACKED4_PROTOTYPES)
    assert raw.oq_qdq_packed4_extension_version() == 1 == _lib.OQ_QDQ_PACKED4_EXTENSION_VERSION
    assert raw.oq_abi_version() == 2 and raw.oq_qdq_extension_version() == 1                                   # additions only
    assert (_lib.OQ_INT4, _lib.OQ_UINT4) == (INT4, UINT4)
    assert "-fno-slp-vectorize" in _build.flags_for("qdq_matmul_packed4.hip")


def test_the_header_is_plain_c99(tmp_path):
    src = tmp_path / "packed4_header.c"
    src.write_text('#include "oq_hip_qdq_packed4.h"\n'
                   "typedef void (*fn)(void);\n"
                   "fn taken[] = {(fn)oq_qdq_packed4_extension_version, (fn)oq_qdq_matmul_packed4_workspace_bytes, (fn)oq_qdq_matmul_packed4};\n"
                   "int codes[] = {OQ_UINT4, OQ_INT4, OQ_TENSOR, OQ_CHANNEL, OQ_GROUP, OQ_QDQ_PACKED4_EXTENSION_VERSION, OQ_ERR_UNSUPPORTED};\n")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                         str(tmp_path / "packed4_header.o")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr


@pytest.mark.parametrize("atype", [F32, F16, BF16])
def test_the_workspace_query_is_that_of_the_byte_route(lib, atype):
    for M, K, N in SHAPES + [(0, 64, 16), (8, 64, 1 << 62)]:
        assert lib.oq_qdq_matmul_packed4_workspace_bytes(M, K, N, atype) == lib.oq_qdq_matmul_workspace_bytes(M, K, N, atype)
    assert lib.oq_qdq_matmul_packed4_workspace_bytes(8, 64, 16, 3) == 0

