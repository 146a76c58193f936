"""The MatMulNBits extension of the C ABI (include/oq_hip_nbits.h): declared, bound and exported as one set, plain C99, its
refusals answer on the host with their status and a message, and its workspace query follows the formula the header states.
oq_hip.h and oq_hip_half.h keep their pins.

Every library call below is one the checks must REFUSE before any device work, so this file is safe on a box with a GPU too:
the pointers are host memory standing in for device memory and nothing may be launched on them."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "oq_hip_nbits.h")
F32, F16, BF16 = 0, 1, 2
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
    assert declared_symbols(HEADER) == sorted(_lib.NBITS_PROTOTYPES)
    assert not set(_lib.NBITS_PROTOTYPES) & (set(_lib.PROTOTYPES) | set(_lib.HALF_PROTOTYPES))
    raw = C.CDLL(lib_path)
    for name in _lib.NBITS_PROTOTYPES:
        assert hasattr(raw, name), f"{name} is declared in include/oq_hip_nbits.h but not exported"
    assert len(_lib.NBITS_PROTOTYPES["oq_matmul_nbits"][1]) == 19
    assert len(_lib.NBITS_PROTOTYPES["oq_matmul_nbits_workspace_bytes"][1]) == 5
    assert raw.oq_nbits_extension_version() == 1 == _lib.OQ_NBITS_EXTENSION_VERSION
    assert (_lib.OQ_NBITS_F32, _lib.OQ_NBITS_F16, _lib.OQ_NBITS_BF16) == (F32, F16, BF16)
    assert raw.oq_abi_version() == 2 and raw.oq_half_extension_version() == 1          # additions only: the pins stay


def test_the_header_is_plain_c99(tmp_path):
    src = tmp_path / "nbits_header.c"
    src.write_text('#include "oq_hip_nbits.h"\n'
                   "typedef void (*fn)(void);\n"
                   "fn taken[] = {(fn)oq_nbits_extension_version, (fn)oq_matmul_nbits_workspace_bytes, (fn)oq_matmul_nbits};\n"
                   "int codes[] = {OQ_NBITS_F32, OQ_NBITS_F16, OQ_NBITS_BF16, OQ_NBITS_EXTENSION_VERSION, OQ_NBITS_FLOAT_ZERO_POINTS,\n"
                   "               OQ_NBITS_G_IDX, OQ_ERR_UNSUPPORTED};\n")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                         str(tmp_path / "nbits_header.o")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr


# ------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def host_ptr():
    buf = (C.c_char * (1 << 18))()
    base = C.addressof(buf)
    yield buf, base + (-base % 256)


def call_args(ptr, **over):
    a = dict(A=ptr, atype=F32, M=8, K=64, lda=64, B=ptr, bits=4, N=16, group_size=32, scales=ptr, scales_type=F32, zero_points=None,
             bias=None, flags=0, Y=ptr, ldy=16, workspace=ptr, workspace_bytes=1 << 17, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
CASES = [
    # (what is hostile, overrides, statuses allowed, a word of the message)
    ("null A", dict(A=None), (INVALID,), "null"), ("null B", dict(B=None), (INVALID,), "null"),
    ("null scales", dict(scales=None), (INVALID,), "null"), ("null Y", dict(Y=None), (INVALID,), "null"),
    ("atype=3", dict(atype=3), (INVALID,), "atype"), ("atype=-1", dict(atype=-1), (INVALID,), "atype"),
    ("fp16 scales for fp32 A", dict(scales_type=F16), (INVALID,), "scales_type"), ("scales_type=9", dict(scales_type=9), (INVALID,), "scales_type"),
    ("M=0", dict(M=0), (INVALID,), "M=0"), ("M=-1", dict(M=-1), (INVALID,), "M=-1"), ("M=2^62", dict(M=HUGE), (INVALID,), "M="),
    ("K=0", dict(K=0), (INVALID,), "K=0"), ("K=-1", dict(K=-1), (INVALID,), "K=-1"), ("K=2^62", dict(K=HUGE, lda=HUGE), (INVALID,), "K="),
    ("N=0", dict(N=0), (INVALID,), "N=0"), ("N=-1", dict(N=-1), (INVALID,), "N=-1"), ("N=2^62", dict(N=HUGE, ldy=HUGE), (INVALID,), "N="),
    ("lda<K", dict(lda=63), (INVALID,), "lda=63"), ("lda=2^62", dict(lda=HUGE), (INVALID,), "lda="),
    ("ldy<N", dict(ldy=15), (INVALID,), "ldy=15"), ("ldy=2^62", dict(ldy=HUGE), (INVALID,), "ldy="),
    ("M*lda>2^40", dict(M=1 << 30, lda=1 << 11), (INVALID,), "outside the bounds"),
    ("M*ldy>2^40", dict(M=1 << 30, ldy=1 << 11), (INVALID,), "outside the bounds"),
    ("N*K>2^40", dict(N=1 << 30, ldy=1 << 30, K=1 << 11, lda=1 << 11, M=1), (INVALID,), "2^40"),
    ("all huge", dict(M=HUGE, K=HUGE, N=HUGE, lda=HUGE, ldy=HUGE, group_size=HUGE, workspace_bytes=1 << 62), (INVALID,), "M="),
    ("bits=2", dict(bits=2), (UNSUPPORTED,), "bits = 2"), ("bits=16", dict(bits=16), (UNSUPPORTED,), "bits = 16"),
    ("g=16", dict(group_size=16), (UNSUPPORTED,), "group_size = 16"), ("g=48", dict(group_size=48), (UNSUPPORTED,), "group_size = 48"),
    ("g=0", dict(group_size=0), (UNSUPPORTED,), "group_size = 0"), ("g=-32", dict(group_size=-32), (UNSUPPORTED,), "group_size"),
    ("float zero points", dict(flags=1), (UNSUPPORTED,), "float zero points"), ("g_idx", dict(flags=2), (UNSUPPORTED,), "g_idx"),
    ("unknown flag", dict(flags=8), (INVALID,), "flags"),
    ("odd A", dict(A="odd"), (INVALID,), "aligned"), ("odd Y", dict(Y="odd"), (INVALID,), "aligned"),
    ("odd scales", dict(scales="odd"), (INVALID,), "aligned"), ("odd bias", dict(bias="odd"), (INVALID,), "aligned"),
    ("B off by 8", dict(B="eight"), (INVALID,), "16-byte"),
    ("null workspace", dict(workspace=None), (WORKSPACE,), "workspace"), ("short workspace", dict(workspace_bytes=64), (WORKSPACE,), "workspace"),
    ("workspace one byte short", dict(workspace_bytes=2 * 1024 + 256 - 1), (WORKSPACE,), "workspace"),
    ("misaligned workspace", dict(workspace="eight"), (WORKSPACE,), "workspace"),
    ("split K without its slabs", dict(atype=F16, scales_type=F16, K=1024, lda=1024, group_size=128, workspace=None), (WORKSPACE,), "workspace"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_matmul_nbits_refuses_on_the_host(lib, host_ptr, case):
    buf, ptr = host_ptr
    _, over, allowed, word = case
    over = {k: (ptr + 1 if v == "odd" else ptr + 8 if v == "eight" else v) for k, v in over.items()}
    before = bytes(buf)
    st = lib.oq_matmul_nbits(*call_args(ptr, **over))
    msg = lib.oq_last_error().decode()
    assert st in allowed, (st, msg)
    assert word in msg, msg
    assert bytes(buf) == before                                   # nothing written on failure


# ------------------------------------------------------------------------------------ the workspace query
def r256(n):
    return (n + 255) // 256 * 256


def stated_formula(M, K, N, atype):
    """include/oq_hip_nbits.h, `workspace`."""
    pieces = 2 * r256(M * 8 * ((K + 7) // 8) * 2) + r256(M * 4) if atype == F32 else 0
    bm = 32 if M <= 32 else 128
    tiles = -(-M // bm) * -(-N // 128)
    steps = -(-K // 64)
    want = 1 if tiles >= 128 else min(8, steps, 256 // tiles)
    splits = -(-steps // -(-steps // want))
    return pieces + (r256(splits * M * N * 4) if splits > 1 else 0)


SHAPES = [(8, 64, 16, 32), (1, 4096, 4096, 128), (16, 4096, 11008, 128), (3, 4096, 64, 128), (70, 1024, 260, 128), (2048, 4096, 4096, 128),
          (33, 100, 17, 32), (17, 11008, 4096, 11008), (1, 32, 1, 32), (129, 6400, 300, 64)]


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
@pytest.mark.parametrize("atype", [F32, F16, BF16])
def test_workspace_query_follows_the_stated_formula(lib, shape, atype):
    M, K, N, g = shape
    assert lib.oq_matmul_nbits_workspace_bytes(M, K, N, g, atype) == stated_formula(M, K, N, atype)


def test_workspace_query_of_a_large_half_product_is_zero_and_its_call_needs_none(lib):
    assert lib.oq_matmul_nbits_workspace_bytes(2048, 4096, 4096, 128, F16) == 0          # no pieces, 512 tiles: no split


QUERY_CASES = [("M=0", (0, 64, 16, 32, F32)), ("M=-1", (-1, 64, 16, 32, F32)), ("M=2^62", (HUGE, 64, 16, 32, F32)), ("K=0", (8, 0, 16, 32, F32)),
               ("K=2^62", (8, HUGE, 16, 32, F32)), ("N=0", (8, 64, 0, 32, F32)), ("N=2^62", (8, 64, HUGE, 32, F32)), ("g=0", (8, 64, 16, 0, F32)),
               ("g=-1", (8, 64, 16, -1, F32)), ("atype=3", (8, 64, 16, 32, 3)), ("M*N>2^40", (1 << 30, 64, 1 << 11, 32, F16)),
               ("M*K>2^40", (1 << 30, 1 << 11, 16, 32, F16)), ("N*K>2^40", (1, 1 << 11, 1 << 30, 32, F16)), ("all huge", (HUGE, HUGE, HUGE, HUGE, F32))]


@pytest.mark.parametrize("case", QUERY_CASES, ids=[c[0] for c in QUERY_CASES])
def test_workspace_query_returns_zero_outside_the_bounds(lib, case):
    assert lib.oq_matmul_nbits_workspace_bytes(*case[1]) == 0
