"""The QDQ function extension of the C ABI (include/oq_hip_qdq_function.h): declared, bound and exported as one set, plain C99, its
refusals answer on the host with their status and a message, and the workspace query follows the formula the header states -- walked
piece by piece by a stand-alone C++ program under AddressSanitizer.  The older extensions keep their pins.

Every library call below is one the checks must REFUSE before any device work, so this file is safe on a box with a GPU too: the
pointers are host memory standing in for device memory and nothing may be launched on them."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_qlinear_function_abi import arguments, declared_symbols

HEADER = os.path.join(ROOT, "include", "oq_hip_qdq_function.h")
NONE, STATIC, DYNAMIC = 0, 1, 2
U8, I8 = 0, 1
F32, F16, BF16 = 0, 1, 2
INT4, UINT4, INT8, UINT8 = 0, 1, 2, 3
TENSOR, CHANNEL, GROUP = 0, 1, 2
HUGE = (1 << 62) + 12345
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


def r256(n):
    return (n + 255) // 256 * 256


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
    assert declared_symbols(HEADER) == sorted(_lib.QDQ_FUNCTION_PROTOTYPES)
    others = [p for p, *_ in _lib.EXTENSIONS if p is not _lib.QDQ_FUNCTION_PROTOTYPES]
    assert len(others) == len(_lib.EXTENSIONS) - 1 and not any(set(_lib.QDQ_FUNCTION_PROTOTYPES) & set(p) for p in others)
    raw = C.CDLL(lib_path)
    for name in _lib.QDQ_FUNCTION_PROTOTYPES:
        assert hasattr(raw, name), f"{name} is declared in include/oq_hip_qdq_function.h but not exported"
    assert raw.oq_qdq_function_extension_version() == 1 == _lib.OQ_QDQ_FUNCTION_EXTENSION_VERSION
    assert (_lib.OQ_QDQ_NONE, _lib.OQ_QDQ_STATIC, _lib.OQ_QDQ_DYNAMIC) == (NONE, STATIC, DYNAMIC)
    assert raw.oq_qdq_extension_version() == 1 and raw.oq_qlinear_function_extension_version() == 1 and raw.oq_abi_version() == 2      # the pins stay


def test_the_header_arguments_match_the_ctypes_prototypes():
    from onnx_quantize_amd.hip import _lib
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t}
    for name, (res, args) in _lib.QDQ_FUNCTION_PROTOTYPES.items():
        declared = [a for a in arguments(HEADER, r"\b" + name) if a != "void"]
        assert len(declared) == len(args), (name, declared)
        for text, bound in zip(declared, args):
            assert bound is (C.c_void_p if "*" in text else ctype[text.split()[0]]), (name, text, bound)
    assert len(_lib.QDQ_FUNCTION_PROTOTYPES["oq_qdq_function"][1]) == 29


def test_the_header_is_plain_c99(tmp_path):
    src = tmp_path / "qdq_function_header.c"
    src.write_text('#include "oq_hip_qdq_function.h"\n'
                   "typedef void (*fn)(void);\n"
                   "fn taken[] = {(fn)oq_qdq_function_extension_version, (fn)oq_qdq_function_workspace_bytes, (fn)oq_qdq_function, (fn)oq_qdq_matmul};\n"
                   "int codes[] = {OQ_QDQ_NONE, OQ_QDQ_STATIC, OQ_QDQ_DYNAMIC, OQ_QL_U8, OQ_QL_I8, OQ_NBITS_F32, OQ_UINT8, OQ_CHANNEL,\n"
                   "               OQ_QDQ_FUNCTION_EXTENSION_VERSION, OQ_QDQ_EXTENSION_VERSION, OQ_ERR_UNSUPPORTED};\n"
                   "int32_t call(const float* x, float* y, const void* w, const float* s, void* ws) {\n"
                   "    return oq_qdq_function(x, OQ_NBITS_F32, 1, 64, 64, OQ_QDQ_DYNAMIC, OQ_QL_U8, 0, 0, w, OQ_INT8, 16, 16, OQ_TENSOR, 0, s, 0, 0, 0, 0,\n"
                   "                           OQ_QDQ_NONE, OQ_QL_U8, 0, 0, y, 16, ws, oq_qdq_function_workspace_bytes(1, 64, 16, OQ_QDQ_DYNAMIC, OQ_QDQ_NONE), 0);\n"
                   "}\n")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                         str(tmp_path / "qdq_function_header.o")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr


# ------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def host_ptr():
    buf = (C.c_char * (1 << 18))()
    base = C.addressof(buf)
    yield buf, base + (-base % 256)


def call_args(ptr, **over):
    # M = 8, K = 2048, N = 16, static in and out: Q + R + C + S = 16384 + 256 + 2048 + 4096 bytes
    a = dict(X=ptr, atype=F32, M=8, K=2048, lda=2048, x_mode=STATIC, x_type=U8, x_scale=ptr, x_zero_point=None, W=ptr, wtype=INT8, N=16, ldw=16,
             granularity=TENSOR, group_size=0, w_scale=ptr, w_zero_point=None, B=None, b_scale=None, b_zero_point=None, out_mode=STATIC, out_type=U8,
             out_scale=ptr, out_zero_point=None, Y=ptr, ldy=16, workspace=ptr, workspace_bytes=1 << 17, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


CASES = [
    # (what is hostile, overrides, status, a word of the message)
    ("null X", dict(X=None), INVALID, "null"), ("null W", dict(W=None), INVALID, "null"), ("null Y", dict(Y=None), INVALID, "null"),
    ("null w_scale", dict(w_scale=None), INVALID, "w_scale"), ("null x_scale, static", dict(x_scale=None), INVALID, "x_scale"),
    ("null out_scale, static", dict(out_scale=None), INVALID, "out_scale"), ("B without b_scale", dict(B="ptr"), INVALID, "b_scale"),
    ("atype=7", dict(atype=7), INVALID, "atype"), ("wtype=9", dict(wtype=9), INVALID, "wtype"), ("wtype=INT32", dict(wtype=4), INVALID, "wtype"),
    ("granularity=3", dict(granularity=3), INVALID, "granularity"),
    ("x_mode=NONE", dict(x_mode=NONE), INVALID, "oq_qdq_matmul"), ("x_mode=3", dict(x_mode=3), INVALID, "x_mode"), ("out_mode=-1", dict(out_mode=-1), INVALID, "out_mode"),
    ("x_type=2", dict(x_type=2), INVALID, "x_type"), ("out_type=5", dict(out_type=5), INVALID, "out_type"),
    ("M=0", dict(M=0), INVALID, "M=0"), ("M=-1", dict(M=-1), INVALID, "M=-1"), ("M=2^62", dict(M=HUGE), INVALID, "M="),
    ("K=0", dict(K=0), INVALID, "K=0"), ("K=2^62", dict(K=HUGE, lda=HUGE), INVALID, "K="),
    ("N=0", dict(N=0), INVALID, "N=0"), ("N=2^62", dict(N=HUGE, ldy=HUGE, ldw=HUGE), INVALID, "N="),
    ("lda<K", dict(lda=2047), INVALID, "lda=2047"), ("ldw<N", dict(ldw=15), INVALID, "ldw=15"), ("ldy<N", dict(ldy=15), INVALID, "ldy=15"),
    ("ldy=2^62", dict(ldy=HUGE), INVALID, "ldy="), ("K*ldw>2^40", dict(N=1 << 30, ldw=1 << 30, ldy=1 << 30, M=1), INVALID, "N=1073741824"),
    ("fp16 X", dict(atype=F16), UNSUPPORTED, "fp16 / bf16 X"), ("bf16 X", dict(atype=BF16), UNSUPPORTED, "fp16 / bf16 X"),
    ("grouped W", dict(granularity=GROUP, group_size=32), UNSUPPORTED, "grouped W"),
    ("uint4 W", dict(wtype=UINT4), UNSUPPORTED, "4-bit W"), ("int4 W", dict(wtype=INT4), UNSUPPORTED, "4-bit W"),
    ("K beyond the int32 sum", dict(K=33026, lda=33026), UNSUPPORTED, "wrap"),
    ("misaligned X", dict(X="odd"), INVALID, "aligned"), ("X two bytes off", dict(X="two"), INVALID, "aligned"),
    ("misaligned Y", dict(Y="two"), INVALID, "aligned"), ("misaligned B", dict(B="odd", b_scale="ptr"), INVALID, "aligned"),
    ("misaligned b_zero_point", dict(B="ptr", b_scale="ptr", b_zero_point="two"), INVALID, "aligned"),
    ("misaligned x_scale", dict(x_scale="odd"), INVALID, "aligned"), ("misaligned w_scale", dict(w_scale="odd"), INVALID, "aligned"),
    ("misaligned out_scale", dict(out_scale="two"), INVALID, "aligned"), ("misaligned b_scale", dict(B="ptr", b_scale="odd"), INVALID, "aligned"),
    ("null workspace", dict(workspace=None), WORKSPACE, "workspace"), ("short workspace", dict(workspace_bytes=64), WORKSPACE, "workspace"),
    ("misaligned workspace", dict(workspace="eight"), WORKSPACE, "workspace"),
    ("workspace one byte short", dict(workspace_bytes=16384 + 256 + 2048 + 4096 - 1), WORKSPACE, "workspace"),
    ("dynamic workspace one byte short", dict(x_mode=DYNAMIC, out_mode=DYNAMIC, workspace_bytes=16384 + 256 + 2048 + 4096 + 256 + 256 + 256 - 1), WORKSPACE,
     "workspace"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_qdq_function_refuses_on_the_host(lib, host_ptr, case):
    buf, ptr = host_ptr
    _, over, expected, word = case
    over = {k: ({"ptr": ptr, "odd": ptr + 1, "two": ptr + 2, "eight": ptr + 8}.get(v, v) if isinstance(v, str) else v) for k, v in over.items()}
    before = bytes(buf)
    st = lib.oq_qdq_function(*call_args(ptr, **over))
    msg = lib.oq_last_error().decode()
    assert st == expected, (st, msg)
    assert word in msg and "oq_qdq_function" in msg, msg
    assert bytes(buf) == before                                   # nothing written on failure


def test_what_a_mode_does_not_read_is_not_required(lib, host_ptr):
    """A dynamic input needs no x_scale and reads no x_type, a dynamic or absent output no out_scale / out_type; rows of X that are
    only 4-byte aligned and a W at any byte are no refusal: such calls get as far as the workspace check, the last before the launch."""
    _, ptr = host_ptr
    for over in (dict(x_mode=DYNAMIC, x_scale=None, x_type=77), dict(out_mode=DYNAMIC, out_scale=None, out_type=-3), dict(out_mode=NONE, out_scale=None),
                 dict(X=ptr + 4), dict(X=ptr + 12, lda=2049), dict(W=ptr + 3, ldw=19), dict(wtype=UINT8, granularity=CHANNEL, x_type=I8, out_type=I8),
                 dict(B=ptr, b_scale=ptr), dict(K=33025, lda=33025)):
        st = lib.oq_qdq_function(*call_args(ptr, workspace=None, **over))
        assert st == WORKSPACE, (over, st, lib.oq_last_error().decode())


# ------------------------------------------------------------------------------------ the workspace query
def test_the_workspace_query_follows_the_stated_formula(lib):
    from qdq_function_cases import workspace
    shapes = [(M, K, N) for M in (1, 16, 32, 33, 129, 2048, 9000) for K, N in ((1, 1), (63, 100), (64, 130), (65, 1), (200, 260), (1088, 130), (4096, 11008),
                                                                              (11008, 4096), (4096, 4096))]
    for M, K, N in shapes:
        for x_mode in (STATIC, DYNAMIC):
            for out_mode in (NONE, STATIC, DYNAMIC):
                got = lib.oq_qdq_function_workspace_bytes(M, K, N, x_mode, out_mode)
                assert got == workspace(M, K, N, x_mode, out_mode), (M, K, N, x_mode, out_mode)
        assert lib.oq_qdq_function_workspace_bytes(M, K, N, STATIC, NONE) == lib.oq_qlinear_function_workspace_bytes(M, K, N)      # Q + R + C + S
    assert lib.oq_qdq_function_workspace_bytes(8, 2048, 16, DYNAMIC, DYNAMIC) == 16384 + 256 + 2048 + 4096 + 256 + 256 + 256


QUERY_CASES = [("M=0", (0, 64, 16, STATIC, NONE)), ("M=2^62", (HUGE, 64, 16, STATIC, NONE)), ("K=0", (8, 0, 16, STATIC, NONE)),
               ("K=33026", (8, 33026, 16, STATIC, NONE)), ("N=0", (8, 64, 0, STATIC, NONE)), ("N=2^62", (8, 64, HUGE, STATIC, NONE)),
               ("x_mode=NONE", (8, 64, 16, NONE, NONE)), ("x_mode=3", (8, 64, 16, 3, NONE)), ("out_mode=3", (8, 64, 16, STATIC, 3)),
               ("out_mode=-1", (8, 64, 16, DYNAMIC, -1))]


@pytest.mark.parametrize("case", QUERY_CASES, ids=[c[0] for c in QUERY_CASES])
def test_the_workspace_query_returns_zero_outside_the_bounds(lib, case):
    assert lib.oq_qdq_function_workspace_bytes(*case[1]) == 0
    assert "oq_qdq_function_workspace_bytes" in lib.oq_last_error().decode()


def test_the_carver_walks_the_formula_under_asan(lib, tmp_path):
    """tests/c/qdq_function_workspace_walk.cpp, a stand-alone program: every piece of every mode inside a heap block of exactly the
    formula's size, and the sizes it prints are the library's."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "qdq_function_workspace_walk")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "onnx_quantize_amd", "csrc"), os.path.join(ROOT, "tests", "c", "qdq_function_workspace_walk.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "walked=66 bad=0"
    for line in lines[:-1]:
        M, K, N, x_mode, out_mode, need = (int(v) for v in line.split())
        assert lib.oq_qdq_function_workspace_bytes(M, K, N, x_mode, out_mode) == need, line
