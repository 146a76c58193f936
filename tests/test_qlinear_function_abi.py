"""The QLinear function extension of the C ABI (include/oq_hip_qlinear_function.h): declared, bound and exported as one set, plain C99,
its refusals answer on the host with their status and a message, and both workspace queries follow the formulas the header states.
The older extensions keep their pins.

Every library call below is one the checks must REFUSE before any device work, so this file is safe on a box with a GPU too:
the pointers are host memory standing in for device memory and nothing may be launched on them."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from qlinear_decode_cases import KN, NK

HEADER = os.path.join(ROOT, "include", "oq_hip_qlinear_function.h")
U8, I8 = 0, 1
HUGE = (1 << 62) + 12345


def r256(n):
    return (n + 255) // 256 * 256


def declared_symbols(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(oq_[a-z0-9_]+)\s*\(", text)))


def arguments(path, name):
    """The argument list of `name` in a header: types and names, comments and line breaks dropped."""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return [re.sub(r"\s+", " ", a).strip() for a in re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")]


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
    assert declared_symbols(HEADER) == sorted(_lib.QLINEAR_FUNCTION_PROTOTYPES)
    others = [p for p, *_ in _lib.EXTENSIONS if p is not _lib.QLINEAR_FUNCTION_PROTOTYPES]
    assert len(others) == len(_lib.EXTENSIONS) - 1 and not any(set(_lib.QLINEAR_FUNCTION_PROTOTYPES) & set(p) for p in others)
    raw = C.CDLL(lib_path)
    for name in _lib.QLINEAR_FUNCTION_PROTOTYPES:
        assert hasattr(raw, name), f"{name} is declared in include/oq_hip_qlinear_function.h but not exported"
    assert raw.oq_qlinear_function_extension_version() == 1 == _lib.OQ_QLINEAR_FUNCTION_EXTENSION_VERSION
    assert raw.oq_qlinear_decode_extension_version() == 1 and raw.oq_qlinear_extension_version() == 1 and raw.oq_abi_version() == 2      # the pins stay


def test_the_header_arguments_match_the_ctypes_prototypes():
    """One ctypes type per declared argument, pointer for pointer and width for width; both entry points take the argument list of
    oq_qlinear_matmul with A and Y as fp32 and `y_type` in the place of `out`."""
    from onnx_quantize_amd.hip import _lib
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t}
    for name, (res, args) in _lib.QLINEAR_FUNCTION_PROTOTYPES.items():
        declared = [a for a in arguments(HEADER, r"\b" + name) if a != "void"]
        assert len(declared) == len(args), (name, declared)
        for text, bound in zip(declared, args):
            assert bound is (C.c_void_p if "*" in text else ctype[text.split()[0]]), (name, text, bound)
    matmul = arguments(os.path.join(ROOT, "include", "oq_hip_qlinear.h"), "int32_t oq_qlinear_matmul")
    expected = [{"const void* A": "const float* A", "int32_t out": "int32_t y_type", "void* Y": "float* Y"}.get(a, a) for a in matmul]
    assert arguments(HEADER, "int32_t oq_qlinear_function") == expected == arguments(HEADER, "int32_t oq_qlinear_function_decode")
    assert _lib.QLINEAR_FUNCTION_PROTOTYPES["oq_qlinear_function"] == _lib.QLINEAR_PROTOTYPES["oq_qlinear_matmul"]
    assert _lib.QLINEAR_FUNCTION_PROTOTYPES["oq_qlinear_function_decode"] == _lib.QLINEAR_DECODE_PROTOTYPES["oq_qlinear_matmul_decode"]


def test_the_header_is_plain_c99(tmp_path):
    src = tmp_path / "qlinear_function_header.c"
    src.write_text('#include "oq_hip_qlinear_function.h"\n'
                   "typedef void (*fn)(void);\n"
                   "fn taken[] = {(fn)oq_qlinear_function_extension_version, (fn)oq_qlinear_function_workspace_bytes, (fn)oq_qlinear_function,\n"
                   "              (fn)oq_qlinear_function_decode_workspace_bytes, (fn)oq_qlinear_function_decode, (fn)oq_qlinear_matmul};\n"
                   "int codes[] = {OQ_QL_U8, OQ_QL_I8, OQ_QL_KN, OQ_QL_NK, OQ_QL_ALPHA, OQ_QLINEAR_FUNCTION_EXTENSION_VERSION,\n"
                   "               OQ_QLINEAR_DECODE_EXTENSION_VERSION, OQ_QLINEAR_EXTENSION_VERSION, OQ_ERR_UNSUPPORTED};\n"
                   "int32_t call(const float* x, float* y, const void* b, const float* s, void* ws) {\n"
                   "    return oq_qlinear_function(x, OQ_QL_U8, 1, 64, 64, s, 0, b, OQ_QL_I8, OQ_QL_KN, 16, 16, s, 0, 0, 0, s, 0, 0, OQ_QL_U8, y, 16, ws,\n"
                   "                               oq_qlinear_function_workspace_bytes(1, 64, 16), 0);\n"
                   "}\n")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                         str(tmp_path / "qlinear_function_header.o")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr


# ------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def host_ptr():
    buf = (C.c_char * (1 << 18))()
    base = C.addressof(buf)
    yield buf, base + (-base % 256)


def call_args(ptr, **over):
    # M = 8, K = 2048, N = 16: the tile route needs Q + R + C + S = 16384 + 256 + 2048 + 4096 bytes, the decode route (NK: two slices) 1024
    a = dict(A=ptr, a_type=U8, M=8, K=2048, lda=2048, a_scale=ptr, a_zero_point=None, B=ptr, b_type=I8, b_layout=NK, N=16, ldb=2048, b_scale=ptr,
             b_zero_point=None, b_per_column=0, C=None, y_scale=ptr, y_zero_point=None, flags=0, y_type=U8, Y=ptr, ldy=16, workspace=ptr,
             workspace_bytes=1 << 17, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
BOTH = [
    # (what is hostile, overrides, status, a word of the message)
    ("null A", dict(A=None), INVALID, "null"), ("null B", dict(B=None), INVALID, "null"), ("null Y", dict(Y=None), INVALID, "null"),
    ("null a_scale", dict(a_scale=None), INVALID, "a_scale"), ("null b_scale", dict(b_scale=None), INVALID, "b_scale"),
    ("null y_scale", dict(y_scale=None), INVALID, "y_scale"),
    ("a_type=5", dict(a_type=5), INVALID, "a_type"), ("b_type=-1", dict(b_type=-1), INVALID, "b_type"),
    ("b_layout=7", dict(b_layout=7), INVALID, "b_layout"), ("y_type=2", dict(y_type=2), INVALID, "y_type"), ("y_type=-1", dict(y_type=-1), INVALID, "y_type"),
    ("unknown flag", dict(flags=8), INVALID, "flags"),
    ("M=0", dict(M=0), INVALID, "M=0"), ("M=-1", dict(M=-1), INVALID, "M=-1"), ("M=2^62", dict(M=HUGE), INVALID, "M="),
    ("K=0", dict(K=0), INVALID, "K=0"), ("K=2^62", dict(K=HUGE, lda=HUGE, ldb=HUGE), INVALID, "K="),
    ("N=0", dict(N=0), INVALID, "N=0"), ("N=2^62", dict(N=HUGE, ldy=HUGE), INVALID, "N="),
    ("lda<K", dict(lda=2047), INVALID, "lda=2047"), ("ldb<K", dict(ldb=2047), INVALID, "ldb=2047"), ("ldb<N in KN", dict(b_layout=KN, ldb=15), INVALID, "ldb=15"),
    ("ldy<N", dict(ldy=15), INVALID, "ldy=15"), ("ldy=2^62", dict(ldy=HUGE), INVALID, "ldy="),
    ("N*ldb>2^40", dict(N=1 << 30, ldy=1 << 30, K=1 << 11, M=1), INVALID, "N=1073741824"),
    ("per-row A", dict(flags=1), UNSUPPORTED, "per-row"), ("transA", dict(flags=2), UNSUPPORTED, "transA"), ("alpha", dict(flags=4), UNSUPPORTED, "alpha"),
    ("every flag", dict(flags=7), UNSUPPORTED, "per-row"),
    ("misaligned A", dict(A="odd"), INVALID, "aligned"), ("A two bytes off", dict(A="two"), INVALID, "aligned"),
    ("misaligned Y", dict(Y="odd"), INVALID, "aligned"), ("Y two bytes off", dict(Y="two"), INVALID, "aligned"),
    ("misaligned C", dict(C="odd"), INVALID, "aligned"), ("misaligned a_scale", dict(a_scale="odd"), INVALID, "aligned"),
    ("misaligned b_scale", dict(b_scale="odd"), INVALID, "aligned"), ("misaligned y_scale", dict(y_scale="odd"), INVALID, "aligned"),
    ("null workspace", dict(workspace=None), WORKSPACE, "workspace"), ("short workspace", dict(workspace_bytes=64), WORKSPACE, "workspace"),
    ("misaligned workspace", dict(workspace="eight"), WORKSPACE, "workspace"),
]
TILE = BOTH + [("workspace one byte short", dict(workspace_bytes=16384 + 256 + 2048 + 4096 - 1), WORKSPACE, "workspace")]
DECODE = BOTH + [("M=17", dict(M=17), UNSUPPORTED, "M = 17 rows"), ("M=2048", dict(M=2048), UNSUPPORTED, "oq_qlinear_function is the route"),
                 ("workspace one byte short", dict(workspace_bytes=2 * 8 * 16 * 4 - 1), WORKSPACE, "workspace"),
                 ("null workspace for the KN slabs", dict(b_layout=KN, ldb=16, workspace=None, workspace_bytes=0), WORKSPACE, "workspace")]


def refused(lib, host_ptr, entry, case):
    buf, ptr = host_ptr
    _, over, expected, word = case
    over = {k: ({"odd": ptr + 1, "two": ptr + 2, "eight": ptr + 8}.get(v, v) if isinstance(v, str) else v) for k, v in over.items()}
    before = bytes(buf)
    st = getattr(lib, entry)(*call_args(ptr, **over))
    msg = lib.oq_last_error().decode()
    assert st == expected, (st, msg)
    assert word in msg and entry in msg, msg
    assert bytes(buf) == before                                   # nothing written on failure


@pytest.mark.parametrize("case", TILE, ids=[c[0] for c in TILE])
def test_qlinear_function_refuses_on_the_host(lib, host_ptr, case):
    refused(lib, host_ptr, "oq_qlinear_function", case)


@pytest.mark.parametrize("case", DECODE, ids=[c[0] for c in DECODE])
def test_qlinear_function_decode_refuses_on_the_host(lib, host_ptr, case):
    refused(lib, host_ptr, "oq_qlinear_function_decode", case)


def test_rows_of_a_that_are_only_4_byte_aligned_are_no_refusal(lib, host_ptr):
    """A needs its element's alignment only: with everything else in order the call gets as far as the workspace check, the last one
    before the launch."""
    _, ptr = host_ptr
    for entry in ("oq_qlinear_function", "oq_qlinear_function_decode"):
        for over in (dict(A=ptr + 4), dict(A=ptr + 12, lda=2049), dict(B=ptr + 3, ldb=2051), dict(y_type=I8, a_type=I8)):
            st = getattr(lib, entry)(*call_args(ptr, workspace=None, **over))
            assert st == WORKSPACE, (entry, over, st, lib.oq_last_error().decode())


# ------------------------------------------------------------------------------------ the workspace queries
def tile_workspace(M, K, N):
    """The header's Q + R + C + S, restated from the header's own words."""
    ceil_div = lambda a, b: -(-a // b)      # noqa: E731
    bm = 32 if M <= 32 else 128
    tiles, steps = ceil_div(M, bm) * ceil_div(N, 128), ceil_div(K, 64)
    want = 1 if tiles >= 128 else min(8, steps, 256 // tiles)
    splits = ceil_div(steps, ceil_div(steps, want))
    q = r256(M * ceil_div(K, 16) * 16)
    return q + r256(M * 4) + 8 * r256(N * 4) + (r256(splits * M * N * 4) if splits > 1 else 0)


def test_the_tile_workspace_query_follows_the_stated_formula(lib):
    from nbits_cases import plan
    shapes = [(M, K, N) for M in (1, 16, 32, 33, 129, 2048) for K, N in ((1, 1), (63, 100), (64, 130), (65, 1), (200, 260), (1088, 130), (4096, 11008),
                                                                        (11008, 4096), (4096, 4096))]
    for M, K, N in shapes:
        got = lib.oq_qlinear_function_workspace_bytes(M, K, N)
        assert got == tile_workspace(M, K, N), (M, K, N)
        assert got == r256(M * ((K + 15) // 16 * 16)) + lib.oq_qlinear_matmul_workspace_bytes(M, K, N)      # Q ahead of the integer route's three
        assert plan(M, K, N).splits >= 1
    assert lib.oq_qlinear_function_workspace_bytes(8, 2048, 16) == 16384 + 256 + 2048 + 4096


@pytest.mark.parametrize("layout", [KN, NK], ids=["KN", "NK"])
def test_the_decode_workspace_query_follows_the_stated_formula(lib, layout):
    from qlinear_decode_cases import workspace
    shapes = [(M, K, N) for M in (1, 2, 4, 5, 8, 9, 16)
              for K, N in ((4096, 4096), (4096, 11008), (11008, 4096), (7, 1), (64, 3), (65, 257), (1024, 256), (1025, 33), (2050, 70), (2600, 1000))]
    for M, K, N in shapes:
        assert lib.oq_qlinear_function_decode_workspace_bytes(M, K, N, layout) == workspace(M, K, N, layout), (M, K, N)
        assert lib.oq_qlinear_function_decode_workspace_bytes(M, K, N, layout) == lib.oq_qlinear_matmul_decode_workspace_bytes(M, K, N, layout)


QUERY_CASES = [("M=0", (0, 64, 16)), ("M=-1", (-1, 64, 16)), ("M=2^62", (HUGE, 64, 16)), ("K=0", (8, 0, 16)), ("K=2^62", (8, HUGE, 16)),
               ("N=0", (8, 64, 0)), ("N=2^62", (8, 64, HUGE)), ("N*K>2^40", (1, 1 << 11, 1 << 30)), ("all huge", (HUGE, HUGE, HUGE))]


@pytest.mark.parametrize("case", QUERY_CASES, ids=[c[0] for c in QUERY_CASES])
def test_workspace_queries_return_zero_outside_the_bounds(lib, case):
    assert lib.oq_qlinear_function_workspace_bytes(*case[1]) == 0
    for layout in (KN, NK):
        assert lib.oq_qlinear_function_decode_workspace_bytes(*case[1], layout) == 0


def test_the_decode_query_also_refuses_17_rows_and_unknown_layouts(lib):
    for args in ((17, 64, 16, KN), (17, 2048, 16, NK), (8, 2048, 16, 2), (8, 2048, 16, -1)):
        assert lib.oq_qlinear_function_decode_workspace_bytes(*args) == 0
    assert lib.oq_qlinear_function_workspace_bytes(17, 2048, 16) > 0
