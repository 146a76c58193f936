"""The decode extension of the packed-nibble QDQ function route (include/oq_hip_qdq_function_packed4_decode.h): declared, bound and
exported as one set with the argument lists of oq_hip_qdq_function.h, and its workspace query answers on the host: the header's sum,
0 where that is 0, and 0 with a message for what the route refuses."""
import ctypes as C
import os

import pytest
from conftest import ROOT
from test_qdq_function_abi import DYNAMIC, NONE, STATIC, declared_symbols, lib, lib_path      # noqa: F401 -- its fixtures

HEADER = os.path.join(ROOT, "include", "oq_hip_qdq_function_packed4_decode.h")
MAX_K = 561433


def test_the_prototypes_are_declared_bound_and_exported(lib_path):
    from onnx_quantize_amd import _build
    from onnx_quantize_amd.hip import _lib, ops
    assert declared_symbols(HEADER) == sorted(_lib.QDQ_FUNCTION_PACKED4_DECODE_PROTOTYPES) == [
        "oq_qdq_function_packed4_decode", "oq_qdq_function_packed4_decode_extension_version", "oq_qdq_function_packed4_decode_workspace_bytes"]
    assert _lib.QDQ_FUNCTION_PACKED4_DECODE_PROTOTYPES["oq_qdq_function_packed4_decode"] == _lib.QDQ_FUNCTION_PROTOTYPES["oq_qdq_function"]
    raw = C.CDLL(lib_path)
    assert all(hasattr(raw, name) for name in _lib.QDQ_FUNCTION_PACKED4_DECODE_PROTOTYPES)
    assert raw.oq_qdq_function_packed4_decode_extension_version() == 1 == _lib.OQ_QDQ_FUNCTION_PACKED4_DECODE_EXTENSION_VERSION
    assert raw.oq_abi_version() == 2 and raw.oq_qdq_function_packed4_extension_version() == 1      # additions only
    assert ops.QDQ_FUNCTION_PACKED4_DECODE_MAX_ROWS == 16
    assert _build.flags_for("qdq_function_packed4_decode.hip") == _build.flags_for("qdq_function_packed4.hip")      # one epilogue, one set of flags


@pytest.mark.parametrize("request_,words", [((17, 64, 8, STATIC, NONE), "M <= 16"), ((4, MAX_K + 1, 8, STATIC, NONE), "K <= 561433"),
                                            ((4, 64, 8, NONE, NONE), "x_mode=0"), ((4, 64, 7, DYNAMIC, DYNAMIC), "an even N")])
def test_the_workspace_query_refuses_on_the_host(lib, request_, words):
    assert lib.oq_qdq_function_packed4_decode_workspace_bytes(*request_) == 0
    msg = lib.oq_last_error().decode()
    assert "oq_qdq_function_packed4_decode_workspace_bytes" in msg and words in msg, msg


def test_the_workspace_is_the_headers_sum(lib):
    query = lib.oq_qdq_function_packed4_decode_workspace_bytes
    assert query(16, 64, 260, STATIC, NONE) == 0                                      # one slice, nothing dynamic: no workspace
    assert query(16, 64, 260, DYNAMIC, DYNAMIC) == 256 + 256 + 256                   # P, PX (4 pairs), PO (3 column blocks)
    # 4096 x 11008 at 16 rows: 86 column blocks want 3 slices -- 1408, 1408, 1280 -- and 16 * 11008 / 256 = 688 finishing workgroups
    assert query(16, 4096, 11008, STATIC, NONE) == 3 * 16 * 11008 * 4
    assert query(16, 4096, 11008, DYNAMIC, DYNAMIC) == 3 * 16 * 11008 * 4 + 256 + 256 + 22 * 256      # 688 pairs: 5504 bytes
    assert query(1, 4096, 11008, STATIC, NONE) == 6 * 11008 * 4                       # up to 4 rows: 6 slices of 704
