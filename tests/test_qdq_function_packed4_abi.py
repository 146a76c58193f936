"""The packed-nibble QDQ function extension of the C ABI (include/oq_hip_qdq_function_packed4.h): declared, bound and exported as one
set with the argument lists of oq_hip_qdq_function.h, and its workspace query answers on the host: the 8-bit route's sum up to this
route's own bound on K, 0 and a message beyond it, for an unknown mode and for an odd N."""
import ctypes as C
import os

import pytest
from conftest import ROOT
from test_qdq_function_abi import DYNAMIC, NONE, STATIC, declared_symbols, lib, lib_path      # noqa: F401 -- its fixtures

HEADER = os.path.join(ROOT, "include", "oq_hip_qdq_function_packed4.h")
MAX_K = 561433


def test_the_prototypes_are_declared_bound_and_exported(lib_path):
    from onnx_quantize_amd import _build
    from onnx_quantize_amd.hip import _lib, ops
    assert declared_symbols(HEADER) == sorted(_lib.QDQ_FUNCTION_PACKED4_PROTOTYPES) == [
        "oq_qdq_function_packed4", "oq_qdq_function_packed4_extension_version", "oq_qdq_function_packed4_workspace_bytes"]
    assert _lib.QDQ_FUNCTION_PACKED4_PROTOTYPES["oq_qdq_function_packed4"] == _lib.QDQ_FUNCTION_PROTOTYPES["oq_qdq_function"]      # one argument list
    raw = C.CDLL(lib_path)
    assert all(hasattr(raw, name) for name in _lib.QDQ_FUNCTION_PACKED4_PROTOTYPES)
    assert raw.oq_qdq_function_packed4_extension_version() == 1 == _lib.OQ_QDQ_FUNCTION_PACKED4_EXTENSION_VERSION
    assert raw.oq_abi_version() == 2 and raw.oq_qdq_function_extension_version() == 1 and raw.oq_qdq_packed4_extension_version() == 1      # additions only
    assert ops.QDQ_FUNCTION_PACKED4_MAX_K == MAX_K == (2 ** 31 - 1) // (255 * 15)
    assert "-packed-fp32-ops" in _build.flags_for("qdq_function_packed4.hip")


@pytest.mark.parametrize("request_,words", [((4, MAX_K + 1, 8, STATIC, NONE), "K <= 561433"), ((4, 64, 8, NONE, NONE), "x_mode=0"),
                                            ((4, 64, 8, STATIC, 3), "out_mode=3"), ((4, 64, 7, DYNAMIC, DYNAMIC), "an even N")])
def test_the_workspace_query_refuses_on_the_host(lib, request_, words):
    assert lib.oq_qdq_function_packed4_workspace_bytes(4, 64, 8, STATIC, NONE) > 0      # a good request clears nothing it should not
    assert lib.oq_qdq_function_packed4_workspace_bytes(*request_) == 0
    msg = lib.oq_last_error().decode()
    assert "oq_qdq_function_packed4_workspace_bytes" in msg and words in msg, msg


def test_the_workspace_is_the_byte_routes_sum_and_reaches_this_routes_bound(lib):
    for M, K, N in [(1, 1, 2), (33, 200, 130), (129, 33025, 264)]:
        for modes in [(STATIC, NONE), (DYNAMIC, DYNAMIC)]:
            need = lib.oq_qdq_function_packed4_workspace_bytes(M, K, N, *modes)
            assert need == lib.oq_qdq_function_workspace_bytes(M, K, N, *modes) > 0
    at_bound = lib.oq_qdq_function_packed4_workspace_bytes(1, MAX_K, 2, STATIC, NONE)
    assert at_bound > 0 and at_bound % 256 == 0
    assert lib.oq_qdq_function_workspace_bytes(1, MAX_K, 2, STATIC, NONE) == 0          # the 8-bit entry point stops at 33025
