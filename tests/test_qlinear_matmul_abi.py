"""The QLinearMatMul / QGemm extension of the C ABI (include/oq_hip_qlinear.h): declared, bound and exported as one set, plain C99,
its refusals answer on the host with their status and a message, and its workspace query follows the formula the header states.
oq_hip.h, oq_hip_half.h and oq_hip_nbits.h keep their pins.

Every library call below is one the checks must REFUSE before any device work, so this file is safe on a box with a GPU too:
the pointers are host memory standing in for device memory and nothing may be launched on them."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "oq_hip_qlinear.h")
U8, I8 = 0, 1
KN, NK = 0, 1
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
    assert declared_symbols(HEADER) == sorted(_lib.QLINEAR_PROTOTYPES)
    assert not set(_lib.QLINEAR_PROTOTYPES) & (set(_lib.PROTOTYPES) | set(_lib.HALF_PROTOTYPES) | set(_lib.NBITS_PROTOTYPES))
    raw = C.CDLL(lib_path)
    for name in _lib.QLINEAR_PROTOTYPES:
        assert hasattr(raw, name), f"{name} is declared in include/oq_hip_qlinear.h but not exported"
    assert len(_lib.QLINEAR_PROTOTYPES["oq_qlinear_matmul"][1]) == 25
    assert len(_lib.QLINEAR_PROTOTYPES["oq_qlinear_matmul_workspace_bytes"][1]) == 3
    assert raw.oq_qlinear_extension_version() == 1 == _lib.OQ_QLINEAR_EXTENSION_VERSION
    assert (_lib.OQ_QL_U8, _lib.OQ_QL_I8, _lib.OQ_QL_KN, _lib.OQ_QL_NK) == (U8, I8, KN, NK)
    assert (_lib.OQ_QL_OUT_I32, _lib.OQ_QL_OUT_F32, _lib.OQ_QL_OUT_U8, _lib.OQ_QL_OUT_I8) == (OUT_I32, OUT_F32, OUT_U8, OUT_I8)
    assert (_lib.OQ_QL_PER_ROW_A, _lib.OQ_QL_TRANS_A, _lib.OQ_QL_ALPHA) == (1, 2, 4)
    assert raw.oq_abi_version() == 2 and raw.oq_half_extension_version() == 1 and raw.oq_nbits_extension_version() == 1      # additions only


def test_the_header_is_plain_c99(tmp_path):
    src = tmp_path / "qlinear_header.c"
    src.write_text('#include "oq_hip_qlinear.h"\n'
                   "typedef void (*fn)(void);\n"
                   "fn taken[] = {(fn)oq_qlinear_extension_version, (fn)oq_qlinear_matmul_workspace_bytes, (fn)oq_qlinear_matmul};\n"
                   "int codes[] = {OQ_QL_U8, OQ_QL_I8, OQ_QL_KN, OQ_QL_NK, OQ_QL_OUT_I32, OQ_QL_OUT_F32, OQ_QL_OUT_U8, OQ_QL_OUT_I8,\n"
                   "               OQ_QL_PER_ROW_A, OQ_QL_TRANS_A, OQ_QL_ALPHA, OQ_QLINEAR_EXTENSION_VERSION, OQ_ERR_UNSUPPORTED};\n")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                         str(tmp_path / "qlinear_header.o")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr


# ------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def host_ptr():
    buf = (C.c_char * (1 << 18))()
    base = C.addressof(buf)
    yield buf, base + (-base % 256)


def call_args(ptr, **over):
    a = dict(A=ptr, a_type=U8, M=8, K=64, lda=64, a_scale=ptr, a_zero_point=ptr, B=ptr, b_type=I8, b_layout=KN, N=16, ldb=16, b_scale=ptr,
             b_zero_point=ptr, b_per_column=1, C=None, y_scale=ptr, y_zero_point=ptr, flags=0, out=OUT_U8, Y=ptr, ldy=16, workspace=ptr,
             workspace_bytes=1 << 17, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
NEED = 256 + 8 * 256                       # 8 x 64 x 16: row sums, column sums; one tile, one step -> no slabs
SPLIT = dict(M=8, K=1024, lda=1024)        # 16 steps, one tile: 8 splits -> slabs of r256(8 * 8 * 16 * 4) = 4096
CASES = [
    # (what is hostile, overrides, status, a word of the message)
    ("null A", dict(A=None), INVALID, "null"), ("null B", dict(B=None), INVALID, "null"), ("null Y", dict(Y=None), INVALID, "null"),
    ("null a_scale", dict(a_scale=None), INVALID, "a_scale"), ("null b_scale", dict(b_scale=None, out=OUT_F32), INVALID, "b_scale"),
    ("null y_scale", dict(y_scale=None), INVALID, "y_scale"), ("null y_scale, int8", dict(y_scale=None, out=OUT_I8), INVALID, "y_scale"),
    ("a_type=2", dict(a_type=2), INVALID, "a_type"), ("a_type=-1", dict(a_type=-1), INVALID, "a_type"),
    ("b_type=2", dict(b_type=2), INVALID, "b_type"), ("b_layout=2", dict(b_layout=2), INVALID, "b_layout"),
    ("b_layout=-1", dict(b_layout=-1), INVALID, "b_layout"), ("out=4", dict(out=4), INVALID, "out"), ("out=-1", dict(out=-1), INVALID, "out"),
    ("unknown flag", dict(flags=8), INVALID, "flags"),
    ("M=0", dict(M=0), INVALID, "M=0"), ("M=2^31", dict(M=1 << 31), INVALID, "M="), ("M=-1", dict(M=-1), INVALID, "M=-1"),
    ("K=0", dict(K=0), INVALID, "K=0"), ("K=2^31", dict(K=1 << 31, lda=1 << 31), INVALID, "K="),
    ("N=0", dict(N=0), INVALID, "N=0"), ("N=2^31", dict(N=1 << 31, ldb=1 << 31, ldy=1 << 31), INVALID, "N="),
    ("lda<K", dict(lda=63), INVALID, "lda=63"), ("lda=2^31", dict(lda=1 << 31), INVALID, "lda="),
    ("ldb<N", dict(ldb=15), INVALID, "ldb=15"), ("ldb<K in NK", dict(b_layout=NK, ldb=63), INVALID, "ldb=63"),
    ("ldb=2^31", dict(ldb=1 << 31), INVALID, "ldb="), ("ldy<N", dict(ldy=15), INVALID, "ldy=15"), ("ldy=2^31", dict(ldy=1 << 31), INVALID, "ldy="),
    ("M*lda>2^40", dict(M=1 << 30, lda=1 << 11), INVALID, "outside the bounds"),
    ("K*ldb>2^40", dict(K=1 << 30, lda=1 << 30, M=1, ldb=1 << 11), INVALID, "outside the bounds"),
    ("N*ldb>2^40 in NK", dict(b_layout=NK, N=1 << 30, ldy=1 << 30, M=1, ldb=1 << 11), INVALID, "outside the bounds"),
    ("M*ldy>2^40", dict(M=1 << 30, ldy=1 << 11), INVALID, "outside the bounds"),
    ("N*K>2^40", dict(N=1 << 30, ldb=1 << 30, ldy=1 << 30, K=1 << 11, lda=1 << 11, M=1), INVALID, "outside the bounds"),
    ("all huge", dict(M=HUGE, K=HUGE, N=HUGE, lda=HUGE, ldb=HUGE, ldy=HUGE, workspace_bytes=1 << 62), INVALID, "M="),
    ("per-row A", dict(flags=1), UNSUPPORTED, "per-row"), ("transA", dict(flags=2), UNSUPPORTED, "transA"),
    ("alpha", dict(flags=4), UNSUPPORTED, "alpha"),
    ("odd a_scale", dict(a_scale="odd"), INVALID, "aligned"), ("odd b_scale", dict(b_scale="odd"), INVALID, "aligned"),
    ("odd y_scale", dict(y_scale="odd"), INVALID, "aligned"), ("odd C", dict(C="odd"), INVALID, "aligned"),
    ("odd int32 Y", dict(Y="odd", out=OUT_I32), INVALID, "aligned"), ("odd fp32 Y", dict(Y="odd", out=OUT_F32), INVALID, "aligned"),
    ("null workspace", dict(workspace=None), WORKSPACE, "workspace"), ("short workspace", dict(workspace_bytes=64), WORKSPACE, "workspace"),
    ("workspace one byte short", dict(workspace_bytes=NEED - 1), WORKSPACE, "workspace"),
    ("misaligned workspace", dict(workspace="eight"), WORKSPACE, "workspace"),
    ("split K without its slabs", dict(workspace_bytes=NEED, **SPLIT), WORKSPACE, "workspace"),
    ("split K one byte short", dict(workspace_bytes=NEED + 4096 - 1, **SPLIT), WORKSPACE, "workspace"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_qlinear_matmul_refuses_on_the_host(lib, host_ptr, case):
    buf, ptr = host_ptr
    _, over, status, word = case
    over = {k: (ptr + 1 if v == "odd" else ptr + 8 if v == "eight" else v) for k, v in over.items()}
    before = bytes(buf)
    st = lib.oq_qlinear_matmul(*call_args(ptr, **over))
    msg = lib.oq_last_error().decode()
    assert st == status, (st, msg)
    assert word in msg, msg
    assert bytes(buf) == before                                   # nothing written on failure


# ------------------------------------------------------------------------------------ the workspace query
def r256(n):
    return (n + 255) // 256 * 256


def stated_formula(M, K, N):
    """include/oq_hip_qlinear.h, `workspace`."""
    bm = 32 if M <= 32 else 128
    tiles = -(-M // bm) * -(-N // 128)
    steps = -(-K // 64)
    want = 1 if tiles >= 128 else min(8, steps, 256 // tiles)
    splits = -(-steps // -(-steps // want))
    return r256(M * 4) + 8 * r256(N * 4) + (r256(splits * M * N * 4) if splits > 1 else 0)


# worked by hand from the header's formula: (shape, splits, bytes)
BY_HAND = [
    ((8, 64, 16), 1, 256 + 8 * 256),                                      # one tile, one step: one split
    ((2048, 4096, 4096), 1, 8192 + 8 * 16384),                            # 16 x 32 = 512 tiles >= 128: one split
    ((16, 4096, 4096), 8, 256 + 8 * 16384 + 8 * 16 * 4096 * 4),           # 32 tiles, 64 steps: want = min(8, 64, 8) = 8 of 8 steps
    ((16, 1088, 260), 6, 256 + 8 * 1280 + 99840),                         # 3 tiles, 17 steps: want 8 -> 3 steps a split -> 6 splits, the last of 2;
                                                                      #   6 * 16 * 260 * 4 = 99840 = 390 * 256
    ((129, 200, 100), 4, 768 + 8 * 512 + 206592),                         # 2 tiles, 4 steps: want = min(8, 4, 128) = 4; 4 * 129 * 100 * 4 = 206400 -> 206592
    ((1, 320, 1), 5, 256 + 8 * 256 + 256),                                # 5 steps: want 5, one step each; 5 * 4 = 20 -> 256
]


@pytest.mark.parametrize("case", BY_HAND, ids=[str(c[0]) for c in BY_HAND])
def test_workspace_query_follows_the_stated_formula(lib, case):
    (M, K, N), splits, nbytes = case
    from nbits_cases import plan
    assert plan(M, K, N).splits == splits
    assert lib.oq_qlinear_matmul_workspace_bytes(M, K, N) == nbytes == stated_formula(M, K, N)


SHAPES = [(1, 4096, 4096), (16, 4096, 11008), (3, 4096, 64), (70, 1024, 260), (33, 100, 17), (17, 11008, 4096), (1, 1, 1), (129, 6400, 300)]


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_workspace_query_on_further_shapes(lib, shape):
    assert lib.oq_qlinear_matmul_workspace_bytes(*shape) == stated_formula(*shape)


QUERY_CASES = [("M=0", (0, 64, 16)), ("M=-1", (-1, 64, 16)), ("M=2^31", (1 << 31, 64, 16)), ("K=0", (8, 0, 16)), ("K=2^31", (8, 1 << 31, 16)),
               ("N=0", (8, 64, 0)), ("N=2^31", (8, 64, 1 << 31)), ("M*N>2^40", (1 << 30, 64, 1 << 11)), ("M*K>2^40", (1 << 30, 1 << 11, 16)),
               ("N*K>2^40", (1, 1 << 11, 1 << 30)), ("all huge", (HUGE, HUGE, HUGE))]


@pytest.mark.parametrize("case", QUERY_CASES, ids=[c[0] for c in QUERY_CASES])
def test_workspace_query_returns_zero_outside_the_bounds(lib, case):
    assert lib.oq_qlinear_matmul_workspace_bytes(*case[1]) == 0
