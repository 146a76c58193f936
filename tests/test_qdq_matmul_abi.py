"""The QDQ extension of the C ABI (include/oq_hip_qdq.h): declared, bound and exported as one set, plain C99, its refusals answer
on the host with their status and a message, and its workspace query follows the formula the header states (that of
oq_hip_nbits.h).  oq_hip.h and the other extensions keep their pins.

Every library call below is one the checks must REFUSE before any device work, so this file is safe on a box with a GPU too:
the pointers are host memory standing in for device memory and nothing may be launched on them."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_matmul_nbits_abi import stated_formula

HEADER = os.path.join(ROOT, "include", "oq_hip_qdq.h")
F32, F16, BF16 = 0, 1, 2
INT8, UINT8 = 2, 3
TENSOR, CHANNEL, GROUP = 0, 1, 2
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
    assert declared_symbols(HEADER) == sorted(_lib.QDQ_PROTOTYPES)
    others = [p for p, *_ in _lib.EXTENSIONS if p is not _lib.QDQ_PROTOTYPES]
    assert len(others) == len(_lib.EXTENSIONS) - 1 and not any(set(_lib.QDQ_PROTOTYPES) & set(p) for p in others)
    raw = C.CDLL(lib_path)
    for name in _lib.QDQ_PROTOTYPES:
        assert hasattr(raw, name), f"{name} is declared in include/oq_hip_qdq.h but not exported"
    assert len(_lib.QDQ_PROTOTYPES["oq_qdq_matmul"][1]) == 20
    assert len(_lib.QDQ_PROTOTYPES["oq_qdq_matmul_workspace_bytes"][1]) == 4
    assert raw.oq_qdq_extension_version() == 1 == _lib.OQ_QDQ_EXTENSION_VERSION
    # the type codes are the existing ones: the header defines no enum of its own
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert "enum" not in text and re.findall(r"#define\s+(\w+)", text) == ["OQ_HIP_QDQ_H", "OQ_QDQ_EXTENSION_VERSION"]
    assert (_lib.OQ_INT8, _lib.OQ_UINT8, _lib.OQ_TENSOR, _lib.OQ_CHANNEL, _lib.OQ_GROUP) == (INT8, UINT8, TENSOR, CHANNEL, GROUP)
    assert raw.oq_abi_version() == 2 and raw.oq_half_extension_version() == 1 and raw.oq_nbits_extension_version() == 1      # additions only
    from onnx_quantize_amd import _build
    assert "-fno-slp-vectorize" in _build.flags_for("qdq_matmul.hip")


def test_the_header_is_plain_c99(tmp_path):
    src = tmp_path / "qdq_header.c"
    src.write_text('#include "oq_hip_qdq.h"\n'
                   "typedef void (*fn)(void);\n"
                   "fn taken[] = {(fn)oq_qdq_extension_version, (fn)oq_qdq_matmul_workspace_bytes, (fn)oq_qdq_matmul};\n"
                   "int codes[] = {OQ_NBITS_F32, OQ_NBITS_F16, OQ_NBITS_BF16, OQ_UINT8, OQ_INT8, OQ_TENSOR, OQ_CHANNEL, OQ_GROUP,\n"
                   "               OQ_QDQ_EXTENSION_VERSION, OQ_ERR_UNSUPPORTED};\n")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                         str(tmp_path / "qdq_header.o")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr


# ------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def host_ptr():
    buf = (C.c_char * (1 << 18))()
    base = C.addressof(buf)
    yield buf, base + (-base % 256)


def call_args(ptr, **over):
    a = dict(A=ptr, atype=F32, M=8, K=64, lda=64, W=ptr, wtype=UINT8, N=16, ldw=16, granularity=GROUP, group_size=32, scales=ptr, scales_type=F32,
             zero_points=None, bias=None, Y=ptr, ldy=16, workspace=ptr, workspace_bytes=1 << 17, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
CASES = [
    # (what is hostile, overrides, statuses allowed, a word of the message)
    ("null A", dict(A=None), (INVALID,), "null"), ("null W", dict(W=None), (INVALID,), "null"),
    ("null scales", dict(scales=None), (INVALID,), "null"), ("null Y", dict(Y=None), (INVALID,), "null"),
    ("atype=3", dict(atype=3), (INVALID,), "atype"), ("atype=-1", dict(atype=-1), (INVALID,), "atype"),
    ("fp16 scales for fp32 A", dict(scales_type=F16), (INVALID,), "scales_type"), ("scales_type=9", dict(scales_type=9), (INVALID,), "scales_type"),
    ("wtype=int4", dict(wtype=0), (INVALID,), "wtype"), ("wtype=9", dict(wtype=9), (INVALID,), "wtype"),
    ("granularity=3", dict(granularity=3), (INVALID,), "granularity"), ("granularity=-1", dict(granularity=-1), (INVALID,), "granularity"),
    ("M=0", dict(M=0), (INVALID,), "M=0"), ("M=-1", dict(M=-1), (INVALID,), "M=-1"), ("M=2^62", dict(M=HUGE), (INVALID,), "M="),
    ("K=0", dict(K=0), (INVALID,), "K=0"), ("K=-1", dict(K=-1), (INVALID,), "K=-1"), ("K=2^62", dict(K=HUGE, lda=HUGE), (INVALID,), "K="),
    ("N=0", dict(N=0), (INVALID,), "N=0"), ("N=-1", dict(N=-1), (INVALID,), "N=-1"), ("N=2^62", dict(N=HUGE, ldy=HUGE, ldw=HUGE), (INVALID,), "N="),
    ("lda<K", dict(lda=63), (INVALID,), "lda=63"), ("lda=2^62", dict(lda=HUGE), (INVALID,), "lda="),
    ("ldy<N", dict(ldy=15), (INVALID,), "ldy=15"), ("ldy=2^62", dict(ldy=HUGE), (INVALID,), "ldy="),
    ("ldw<N", dict(ldw=15), (INVALID,), "ldw=15"), ("ldw=2^62", dict(ldw=HUGE), (INVALID,), "ldw="),
    ("M*lda>2^40", dict(M=1 << 30, lda=1 << 11), (INVALID,), "outside the bounds"),
    ("M*ldy>2^40", dict(M=1 << 30, ldy=1 << 11), (INVALID,), "outside the bounds"),
    ("K*ldw>2^40", dict(K=1 << 30, lda=1 << 30, ldw=1 << 11, M=1), (INVALID,), "outside the bounds"),
    ("N*K>2^40", dict(N=1 << 30, ldy=1 << 30, ldw=1 << 30, K=1 << 11, lda=1 << 11, M=1), (INVALID,), "outside the bounds"),
    ("all huge", dict(M=HUGE, K=HUGE, N=HUGE, lda=HUGE, ldy=HUGE, ldw=HUGE, group_size=HUGE, workspace_bytes=1 << 62), (INVALID,), "M="),
    ("g=16", dict(group_size=16), (UNSUPPORTED,), "group_size = 16"), ("g=48", dict(group_size=48), (UNSUPPORTED,), "group_size = 48"),
    ("g=0", dict(group_size=0), (UNSUPPORTED,), "group_size = 0"), ("g=-32", dict(group_size=-32), (UNSUPPORTED,), "group_size"),
    ("K % g", dict(K=96, lda=96, group_size=64), (UNSUPPORTED,), "K = 96 is no multiple of group_size = 64"),
    ("g > K", dict(group_size=128), (UNSUPPORTED,), "no multiple of group_size"),
    ("odd A", dict(A="odd"), (INVALID,), "aligned"), ("odd Y", dict(Y="odd"), (INVALID,), "aligned"),
    ("odd scales", dict(scales="odd"), (INVALID,), "aligned"), ("odd bias", dict(bias="odd"), (INVALID,), "aligned"),
    ("null workspace", dict(workspace=None), (WORKSPACE,), "workspace"), ("short workspace", dict(workspace_bytes=64), (WORKSPACE,), "workspace"),
    ("workspace one byte short", dict(workspace_bytes=2 * 1024 + 256 - 1), (WORKSPACE,), "workspace"),
    ("misaligned workspace", dict(workspace="eight"), (WORKSPACE,), "workspace"),
    ("split K without its slabs", dict(atype=F16, scales_type=F16, K=1024, lda=1024, group_size=128, workspace=None), (WORKSPACE,), "workspace"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_qdq_matmul_refuses_on_the_host(lib, host_ptr, case):
    buf, ptr = host_ptr
    _, over, allowed, word = case
    over = {k: (ptr + 1 if v == "odd" else ptr + 8 if v == "eight" else v) for k, v in over.items()}
    before = bytes(buf)
    st = lib.oq_qdq_matmul(*call_args(ptr, **over))
    msg = lib.oq_last_error().decode()
    assert st in allowed, (st, msg)
    assert word in msg, msg
    assert bytes(buf) == before                                   # nothing written on failure


def test_the_group_size_is_read_for_groups_only(lib, host_ptr):
    """Per tensor / per column no group size is refused: the first thing wrong with these calls is their workspace."""
    _, ptr = host_ptr
    for granularity in (TENSOR, CHANNEL):
        for g in (0, 16, -5):
            st = lib.oq_qdq_matmul(*call_args(ptr, granularity=granularity, group_size=g, workspace=None))
            assert st == WORKSPACE, (granularity, g, lib.oq_last_error())


# ------------------------------------------------------------------------------------ the workspace query
SHAPES = [(8, 64, 16), (1, 4096, 4096), (16, 4096, 11008), (3, 4096, 64), (70, 1024, 260), (2048, 4096, 4096), (33, 100, 17),
          (17, 11008, 4096), (1, 1, 1), (129, 6400, 300)]


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
@pytest.mark.parametrize("atype", [F32, F16, BF16])
def test_workspace_query_follows_the_stated_formula(lib, shape, atype):
    """include/oq_hip_qdq.h, `workspace`: the P + S of oq_hip_nbits.h -- and what oq_matmul_nbits asks for the same product."""
    M, K, N = shape
    assert lib.oq_qdq_matmul_workspace_bytes(M, K, N, atype) == stated_formula(M, K, N, atype)
    assert lib.oq_qdq_matmul_workspace_bytes(M, K, N, atype) == lib.oq_matmul_nbits_workspace_bytes(M, K, N, 32, atype)


QUERY_CASES = [("M=0", (0, 64, 16, F32)), ("M=-1", (-1, 64, 16, F32)), ("M=2^62", (HUGE, 64, 16, F32)), ("K=0", (8, 0, 16, F32)),
               ("K=2^62", (8, HUGE, 16, F32)), ("N=0", (8, 64, 0, F32)), ("N=2^62", (8, 64, HUGE, F32)), ("atype=3", (8, 64, 16, 3)),
               ("M*N>2^40", (1 << 30, 64, 1 << 11, F16)), ("M*K>2^40", (1 << 30, 1 << 11, 16, F16)), ("N*K>2^40", (1, 1 << 11, 1 << 30, F16)),
               ("all huge", (HUGE, HUGE, HUGE, F32))]


@pytest.mark.parametrize("case", QUERY_CASES, ids=[c[0] for c in QUERY_CASES])
def test_workspace_query_returns_zero_outside_the_bounds(lib, case):
    assert lib.oq_qdq_matmul_workspace_bytes(*case[1]) == 0
