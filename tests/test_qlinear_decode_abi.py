"""The QLinearMatMul / QGemm decode extension of the C ABI (include/oq_hip_qlinear_decode.h): declared, bound and exported as one set,
plain C99, its refusals answer on the host with their status and a message, its workspace query follows the formula the header
states, and the launch plan covers every k and every column exactly once (tests/c/qlinear_decode_plan_walk.cpp, under
AddressSanitizer).  oq_hip_qlinear.h keeps its pin.

Every library call below is one the checks must REFUSE before any device work, so this file is safe on a box with a GPU too:
the pointers are host memory standing in for device memory and nothing may be launched on them."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from qlinear_decode_cases import KN, NK, plan, r256, workspace

HEADER = os.path.join(ROOT, "include", "oq_hip_qlinear_decode.h")
CSRC = os.path.join(ROOT, "onnx_quantize_amd", "csrc")
WALK = os.path.join(ROOT, "tests", "c", "qlinear_decode_plan_walk.cpp")
U8, I8 = 0, 1
OUT_I32, OUT_F32, OUT_U8, OUT_I8 = range(4)
HUGE = (1 << 62) + 12345


def declared_symbols(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(oq_[a-z0-9_]+)\s*\(", text)))


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
    assert declared_symbols(HEADER) == sorted(_lib.QLINEAR_DECODE_PROTOTYPES)
    others = (set(_lib.PROTOTYPES) | set(_lib.HALF_PROTOTYPES) | set(_lib.NBITS_PROTOTYPES) | set(_lib.NBITS_DECODE_PROTOTYPES)
              | set(_lib.QLINEAR_PROTOTYPES))
    assert not set(_lib.QLINEAR_DECODE_PROTOTYPES) & others
    raw = C.CDLL(lib_path)
    for name in _lib.QLINEAR_DECODE_PROTOTYPES:
        assert hasattr(raw, name), f"{name} is declared in include/oq_hip_qlinear_decode.h but not exported"
    # exactly the argument list of oq_qlinear_matmul; the query takes the layout as a fourth argument
    assert _lib.QLINEAR_DECODE_PROTOTYPES["oq_qlinear_matmul_decode"] == _lib.QLINEAR_PROTOTYPES["oq_qlinear_matmul"]
    assert len(_lib.QLINEAR_DECODE_PROTOTYPES["oq_qlinear_matmul_decode_workspace_bytes"][1]) == 4
    assert raw.oq_qlinear_decode_extension_version() == 1 == _lib.OQ_QLINEAR_DECODE_EXTENSION_VERSION
    assert raw.oq_qlinear_extension_version() == 1 == _lib.OQ_QLINEAR_EXTENSION_VERSION                  # the pins stay
    assert raw.oq_abi_version() == 2 and raw.oq_nbits_decode_extension_version() == 1


def test_the_argument_lists_of_the_two_entry_points_are_the_same_text():
    def arguments(path, name):
        text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        return re.sub(r"\s+", " ", re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1))
    assert arguments(HEADER, "int32_t oq_qlinear_matmul_decode") == arguments(os.path.join(ROOT, "include", "oq_hip_qlinear.h"), "int32_t oq_qlinear_matmul")


def test_the_header_is_plain_c99(tmp_path):
    src = tmp_path / "qlinear_decode_header.c"
    src.write_text('#include "oq_hip_qlinear_decode.h"\n'
                   "typedef void (*fn)(void);\n"
                   "fn taken[] = {(fn)oq_qlinear_decode_extension_version, (fn)oq_qlinear_matmul_decode_workspace_bytes, (fn)oq_qlinear_matmul_decode,\n"
                   "              (fn)oq_qlinear_matmul};\n"
                   "int codes[] = {OQ_QL_U8, OQ_QL_I8, OQ_QL_KN, OQ_QL_NK, OQ_QL_OUT_I8, OQ_QL_ALPHA, OQ_QLINEAR_DECODE_EXTENSION_VERSION,\n"
                   "               OQ_QLINEAR_EXTENSION_VERSION, OQ_ERR_UNSUPPORTED};\n")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                         str(tmp_path / "qlinear_decode_header.o")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr


# ------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def host_ptr():
    buf = (C.c_char * (1 << 18))()
    base = C.addressof(buf)
    yield buf, base + (-base % 256)


def call_args(ptr, **over):
    # K = 2048 in NK: two slices, S = 2 * 8 * 16 * 4 = 1024 bytes
    a = dict(A=ptr, a_type=U8, M=8, K=2048, lda=2048, a_scale=ptr, a_zero_point=None, B=ptr, b_type=I8, b_layout=NK, N=16, ldb=2048, b_scale=ptr,
             b_zero_point=None, b_per_column=0, C=None, y_scale=ptr, y_zero_point=None, flags=0, out=OUT_U8, Y=ptr, ldy=16, workspace=ptr,
             workspace_bytes=1 << 17, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
CASES = [
    # (what is hostile, overrides, status, a word of the message)
    ("null A", dict(A=None), INVALID, "null"), ("null B", dict(B=None), INVALID, "null"), ("null Y", dict(Y=None), INVALID, "null"),
    ("null a_scale", dict(a_scale=None), INVALID, "a_scale"), ("null b_scale", dict(b_scale=None), INVALID, "b_scale"),
    ("null y_scale", dict(y_scale=None), INVALID, "y_scale"),
    ("a_type=5", dict(a_type=5), INVALID, "a_type"), ("b_type=-1", dict(b_type=-1), INVALID, "b_type"),
    ("b_layout=7", dict(b_layout=7), INVALID, "b_layout"), ("out=9", dict(out=9), INVALID, "out"),
    ("unknown flag", dict(flags=8), INVALID, "flags"),
    ("M=0", dict(M=0), INVALID, "M=0"), ("M=-1", dict(M=-1), INVALID, "M=-1"), ("M=2^62", dict(M=HUGE), INVALID, "M="),
    ("K=0", dict(K=0), INVALID, "K=0"), ("K=2^62", dict(K=HUGE, lda=HUGE, ldb=HUGE), INVALID, "K="),
    ("N=0", dict(N=0), INVALID, "N=0"), ("N=2^62", dict(N=HUGE, ldy=HUGE), INVALID, "N="),
    ("lda<K", dict(lda=2047), INVALID, "lda=2047"), ("ldb<K", dict(ldb=2047), INVALID, "ldb=2047"), ("ldb<N in KN", dict(b_layout=KN, ldb=15), INVALID, "ldb=15"),
    ("ldy<N", dict(ldy=15), INVALID, "ldy=15"), ("ldy=2^62", dict(ldy=HUGE), INVALID, "ldy="),
    ("N*ldb>2^40", dict(N=1 << 30, ldy=1 << 30, K=1 << 11, M=1), INVALID, "N=1073741824"),
    ("M=17", dict(M=17), UNSUPPORTED, "M = 17 rows"), ("M=2048", dict(M=2048), UNSUPPORTED, "oq_qlinear_matmul is the route"),
    ("per-row A", dict(flags=1), UNSUPPORTED, "per-row"), ("transA", dict(flags=2), UNSUPPORTED, "transA"), ("alpha", dict(flags=4), UNSUPPORTED, "alpha"),
    ("every flag", dict(flags=7), UNSUPPORTED, "per-row"),
    ("misaligned Y", dict(Y="odd", out=OUT_I32), INVALID, "aligned"), ("misaligned Y (fp32)", dict(Y="odd", out=OUT_F32), INVALID, "aligned"),
    ("misaligned C", dict(C="odd"), INVALID, "aligned"), ("misaligned a_scale", dict(a_scale="odd"), INVALID, "aligned"),
    ("misaligned b_scale", dict(b_scale="odd"), INVALID, "aligned"), ("misaligned y_scale", dict(y_scale="odd"), INVALID, "aligned"),
    ("null workspace", dict(workspace=None), WORKSPACE, "workspace"), ("short workspace", dict(workspace_bytes=64), WORKSPACE, "workspace"),
    ("workspace one byte short", dict(workspace_bytes=2 * 8 * 16 * 4 - 1), WORKSPACE, "workspace"),
    ("misaligned workspace", dict(workspace="eight"), WORKSPACE, "workspace"),
    ("null workspace for the KN slabs", dict(b_layout=KN, ldb=16, workspace=None, workspace_bytes=0), WORKSPACE, "workspace"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_qlinear_matmul_decode_refuses_on_the_host(lib, host_ptr, case):
    buf, ptr = host_ptr
    _, over, expected, word = case
    over = {k: (ptr + 1 if v == "odd" else ptr + 8 if v == "eight" else v) for k, v in over.items()}
    before = bytes(buf)
    st = lib.oq_qlinear_matmul_decode(*call_args(ptr, **over))
    msg = lib.oq_last_error().decode()
    assert st == expected, (st, msg)
    assert word in msg and "oq_qlinear_matmul_decode" in msg, msg
    assert bytes(buf) == before                                   # nothing written on failure


def test_odd_operand_bases_are_no_refusal(lib, host_ptr):
    """A and B may lie at any byte: with everything else in order the call gets as far as the workspace check, the last one before the
    launch."""
    _, ptr = host_ptr
    for over in (dict(A=ptr + 1), dict(B=ptr + 3), dict(lda=2049, ldb=2051), dict(out=OUT_I32, a_scale=None, b_scale=None, y_scale=None)):
        st = lib.oq_qlinear_matmul_decode(*call_args(ptr, workspace=None, **over))
        assert st == WORKSPACE, (over, st, lib.oq_last_error().decode())


# ------------------------------------------------------------------------------------ the workspace query
SHAPES = [(M, K, N) for M in (1, 2, 4, 5, 8, 9, 16)
          for K, N in ((4096, 4096), (4096, 11008), (11008, 4096), (7, 1), (64, 3), (65, 257), (1024, 256), (1025, 33), (2050, 70), (2600, 1000))]


@pytest.mark.parametrize("layout", [KN, NK], ids=["KN", "NK"])
def test_workspace_query_follows_the_stated_formula(lib, layout):
    for M, K, N in SHAPES:
        assert lib.oq_qlinear_matmul_decode_workspace_bytes(M, K, N, layout) == workspace(M, K, N, layout), (M, K, N)


def test_one_slice_needs_no_workspace_and_model_sizes_need_their_slabs(lib):
    assert lib.oq_qlinear_matmul_decode_workspace_bytes(16, 1024, 4096, NK) == 0 == workspace(16, 1024, 4096, NK)
    assert lib.oq_qlinear_matmul_decode_workspace_bytes(16, 64, 65536, KN) == 0 == workspace(16, 64, 65536, KN)
    assert lib.oq_qlinear_matmul_decode_workspace_bytes(16, 11008, 4096, NK) == 11 * 16 * 4096 * 4
    assert plan(16, 11008, 4096, KN).splits == 16 and plan(1, 11008, 4096, KN).splits == 29
    assert lib.oq_qlinear_matmul_decode_workspace_bytes(16, 11008, 4096, KN) == 16 * 16 * 4096 * 4
    assert lib.oq_qlinear_matmul_decode_workspace_bytes(1, 11008, 4096, KN) == r256(29 * 4096 * 4)
    # the model widths: one to two workgroups per compute unit, both layouts
    for K, N in ((4096, 11008), (11008, 4096), (4096, 4096)):
        for layout in (KN, NK):
            for M in (1, 16):
                assert 192 <= plan(M, K, N, layout).grid <= 640, (M, K, N, layout, plan(M, K, N, layout))


QUERY_CASES = [("M=0", (0, 64, 16, KN)), ("M=-1", (-1, 64, 16, NK)), ("M=17", (17, 64, 16, KN)), ("M=17 NK", (17, 2048, 16, NK)),
               ("M=2^62", (HUGE, 64, 16, KN)), ("K=0", (8, 0, 16, NK)), ("K=2^62", (8, HUGE, 16, KN)), ("N=0", (8, 64, 0, KN)),
               ("N=2^62", (8, 64, HUGE, NK)), ("layout=2", (8, 2048, 16, 2)), ("layout=-1", (8, 2048, 16, -1)),
               ("N*K>2^40", (1, 1 << 11, 1 << 30, NK)), ("all huge", (HUGE, HUGE, HUGE, KN))]


@pytest.mark.parametrize("case", QUERY_CASES, ids=[c[0] for c in QUERY_CASES])
def test_workspace_query_returns_zero_outside_the_bounds(lib, case):
    assert lib.oq_qlinear_matmul_decode_workspace_bytes(*case[1]) == 0


# ------------------------------------------------------------------------------------ the plan, walked
def test_the_plan_covers_every_k_and_every_column_once_under_asan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    text = open(WALK).read()
    assert sorted(re.findall(r'#include "([^"]+)"', text)) == ["qlinear_decode_plan.hpp", "workspace.hpp"]
    exe = str(tmp_path / "qlinear_decode_plan_walk")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, WALK, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "bad=0" in r.stdout and "walked=3332" in r.stdout and "nbits_walked=1904" in r.stdout      # 4 M x 17 K x 14 N x 2 types of A
