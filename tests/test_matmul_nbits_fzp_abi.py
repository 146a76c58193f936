"""The float-zero-point extension of the C ABI (include/oq_hip_nbits_fzp.h): declared, bound and exported as one set, plain C99,
its refusals answer on the host with their status and a message, and its workspace query follows the formula the header states
(P + S of oq_matmul_nbits: the row sums live in registers).  The older headers keep their pins.

Every library call below is one the checks must REFUSE before any device work, so this file is safe on a box with a GPU too:
the pointers are host memory standing in for device memory and nothing may be launched on them."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from nbits_cases import plan, r256

HEADER = os.path.join(ROOT, "include", "oq_hip_nbits_fzp.h")
F32, F16, BF16, ZP_U8 = 0, 1, 2, 3
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
    assert declared_symbols(HEADER) == sorted(_lib.NBITS_FZP_PROTOTYPES)
    assert sorted(_lib.NBITS_FZP_PROTOTYPES) == ["oq_matmul_nbits_fzp", "oq_matmul_nbits_fzp_workspace_bytes", "oq_nbits_fzp_extension_version"]
    others = set(_lib.PROTOTYPES) | set(_lib.HALF_PROTOTYPES) | set(_lib.NBITS_PROTOTYPES) | set(_lib.NBITS_DECODE_PROTOTYPES)
    assert not set(_lib.NBITS_FZP_PROTOTYPES) & others
    raw = C.CDLL(lib_path)
    for name in _lib.NBITS_FZP_PROTOTYPES:
        assert hasattr(raw, name), f"{name} is declared in include/oq_hip_nbits_fzp.h but not exported"
    # the argument list of oq_matmul_nbits_decode
    assert _lib.NBITS_FZP_PROTOTYPES["oq_matmul_nbits_fzp"] == _lib.NBITS_DECODE_PROTOTYPES["oq_matmul_nbits_decode"]
    assert _lib.NBITS_FZP_PROTOTYPES["oq_matmul_nbits_fzp_workspace_bytes"] == _lib.NBITS_PROTOTYPES["oq_matmul_nbits_workspace_bytes"]
    assert raw.oq_nbits_fzp_extension_version() == 1 == _lib.OQ_NBITS_FZP_EXTENSION_VERSION
    assert raw.oq_abi_version() == 2 and raw.oq_nbits_extension_version() == 1 and raw.oq_nbits_decode_extension_version() == 1      # the pins stay


def test_the_header_is_plain_c99(tmp_path):
    src = tmp_path / "nbits_fzp_header.c"
    src.write_text('#include "oq_hip_nbits_fzp.h"\n'
                   "typedef void (*fn)(void);\n"
                   "fn taken[] = {(fn)oq_nbits_fzp_extension_version, (fn)oq_matmul_nbits_fzp_workspace_bytes, (fn)oq_matmul_nbits_fzp,\n"
                   "              (fn)oq_matmul_nbits_decode, (fn)oq_matmul_nbits};\n"
                   "int codes[] = {OQ_NBITS_F32, OQ_NBITS_F16, OQ_NBITS_BF16, OQ_NBITS_ZP_PACKED_U8, OQ_NBITS_FZP_EXTENSION_VERSION,\n"
                   "               OQ_NBITS_FLOAT_ZERO_POINTS, OQ_NBITS_G_IDX, OQ_ERR_UNSUPPORTED};\n"
                   "int32_t call(void) {\n"
                   "    return oq_matmul_nbits_fzp(0, OQ_NBITS_F16, 1, 32, 32, 0, 4, 1, 32, 0, OQ_NBITS_F32, 0, OQ_NBITS_F32, 0,\n"
                   "                               OQ_NBITS_FLOAT_ZERO_POINTS, 0, 1, 0, oq_matmul_nbits_fzp_workspace_bytes(1, 32, 1, 32, OQ_NBITS_F16), 0);\n"
                   "}\n")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                         str(tmp_path / "nbits_fzp_header.o")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr


# ------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def host_ptr():
    buf = (C.c_char * (1 << 18))()
    base = C.addressof(buf)
    yield buf, base + (-base % 256)


def call_args(ptr, **over):
    a = dict(A=ptr, atype=F32, M=8, K=2048, lda=2048, B=ptr, bits=4, N=16, group_size=32, scales=ptr, scales_type=F32, zero_points=ptr,
             zero_points_type=F32, bias=None, flags=1, Y=ptr, ldy=16, workspace=ptr, workspace_bytes=1 << 17, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
# the workspace of the call above: P = 2 * r256(8 * 2048 * 2) + r256(32), S = 8 slabs of 8 x 16 fp32 (one tile, 32 steps: 8 splits)
NEED = 2 * r256(8 * 2048 * 2) + r256(8 * 4) + r256(8 * 8 * 16 * 4)
CASES = [
    # (what is hostile, overrides, status, a word of the message)
    ("null A", dict(A=None), INVALID, "null"), ("null B", dict(B=None), INVALID, "null"),
    ("null scales", dict(scales=None), INVALID, "null"), ("null Y", dict(Y=None), INVALID, "null"),
    ("atype=3", dict(atype=3), INVALID, "atype"), ("atype=-1", dict(atype=-1), INVALID, "atype"),
    ("fp16 scales for fp32 A", dict(scales_type=F16), INVALID, "scales_type"), ("scales_type=9", dict(scales_type=9), INVALID, "scales_type"),
    ("fp16 zero points for fp32 A", dict(zero_points_type=F16), INVALID, "zero_points_type"),
    ("zero_points_type=7", dict(zero_points_type=7), INVALID, "zero_points_type"),
    ("M=0", dict(M=0), INVALID, "M=0"), ("M=-1", dict(M=-1), INVALID, "M=-1"), ("M=2^62", dict(M=HUGE), INVALID, "M="),
    ("K=0", dict(K=0), INVALID, "K=0"), ("K=-1", dict(K=-1), INVALID, "K=-1"), ("K=2^62", dict(K=HUGE, lda=HUGE), INVALID, "K="),
    ("N=0", dict(N=0), INVALID, "N=0"), ("N=-1", dict(N=-1), INVALID, "N=-1"), ("N=2^62", dict(N=HUGE, ldy=HUGE), INVALID, "N="),
    ("lda<K", dict(lda=2047), INVALID, "lda=2047"), ("lda=2^62", dict(lda=HUGE), INVALID, "lda="),
    ("ldy<N", dict(ldy=15), INVALID, "ldy=15"), ("ldy=2^62", dict(ldy=HUGE), INVALID, "ldy="),
    ("N*K>2^40", dict(N=1 << 30, ldy=1 << 30, K=1 << 11, lda=1 << 11, M=1), INVALID, "2^40"),
    ("all huge", dict(M=HUGE, K=HUGE, N=HUGE, lda=HUGE, ldy=HUGE, group_size=HUGE, workspace_bytes=1 << 62), INVALID, "M="),
    ("bits=3", dict(bits=3), UNSUPPORTED, "bits = 3"), ("bits=2", dict(bits=2), UNSUPPORTED, "bits = 2"), ("bits=16", dict(bits=16), UNSUPPORTED, "bits = 16"),
    ("g=16", dict(group_size=16), UNSUPPORTED, "group_size = 16"), ("g=48", dict(group_size=48), UNSUPPORTED, "group_size = 48"),
    ("g=0", dict(group_size=0), UNSUPPORTED, "group_size = 0"), ("g=-32", dict(group_size=-32), UNSUPPORTED, "group_size"),
    ("g_idx", dict(flags=2), UNSUPPORTED, "g_idx"), ("g_idx and float", dict(flags=3), UNSUPPORTED, "g_idx"),
    ("unknown flag", dict(flags=8), INVALID, "flags"),
    ("packed uint8 zero points", dict(zero_points_type=ZP_U8, flags=0), UNSUPPORTED, "packed uint8"),
    ("NULL zero points", dict(zero_points=None, flags=0), UNSUPPORTED, "NULL"),
    ("NULL zero points said to be packed", dict(zero_points=None, zero_points_type=ZP_U8, flags=0), UNSUPPORTED, "oq_matmul_nbits is their route"),
    ("odd A", dict(A="odd"), INVALID, "aligned"), ("odd Y", dict(Y="odd"), INVALID, "aligned"),
    ("odd scales", dict(scales="odd"), INVALID, "aligned"), ("odd bias", dict(bias="odd"), INVALID, "aligned"),
    ("odd zero points", dict(zero_points="odd"), INVALID, "zero_points must be aligned"),
    ("zero points off by 2 for fp32", dict(zero_points="two"), INVALID, "zero_points must be aligned"),
    ("odd fp16 zero points", dict(atype=F16, zero_points_type=F16, zero_points="odd"), INVALID, "zero_points must be aligned"),
    ("odd fp16 scales", dict(atype=F16, scales_type=F16, scales="odd"), INVALID, "aligned"),
    ("B off by 8", dict(B="eight"), INVALID, "16-byte"),
    ("null workspace", dict(workspace=None), WORKSPACE, "workspace"), ("short workspace", dict(workspace_bytes=64), WORKSPACE, "workspace"),
    ("workspace one byte short", dict(workspace_bytes=NEED - 1), WORKSPACE, "workspace"),
    ("misaligned workspace", dict(workspace="eight"), WORKSPACE, "workspace"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_matmul_nbits_fzp_refuses_on_the_host(lib, host_ptr, case):
    buf, ptr = host_ptr
    _, over, expected, word = case
    over = {k: (ptr + 1 if v == "odd" else ptr + 2 if v == "two" else ptr + 8 if v == "eight" else v) for k, v in over.items()}
    before = bytes(buf)
    st = lib.oq_matmul_nbits_fzp(*call_args(ptr, **over))
    msg = lib.oq_last_error().decode()
    assert st == expected, (st, msg)
    assert word in msg and "oq_matmul_nbits_fzp" in msg, msg
    assert bytes(buf) == before                                   # nothing written on failure


def test_the_workspace_of_the_refusal_cases_is_the_one_their_check_wants(lib):
    assert lib.oq_matmul_nbits_fzp_workspace_bytes(8, 2048, 16, 32, F32) == NEED


def test_oq_matmul_nbits_still_refuses_float_zero_points(lib, host_ptr):
    _, ptr = host_ptr
    st = lib.oq_matmul_nbits(ptr, F16, 8, 64, 64, ptr, 4, 16, 32, ptr, F32, None, None, 1, ptr, 16, ptr, 1 << 16, None)
    assert st == UNSUPPORTED and "float zero points" in lib.oq_last_error().decode()


# ------------------------------------------------------------------------------------ the workspace query
def stated_formula(M, K, N, atype):
    """include/oq_hip_nbits_fzp.h, `workspace`: P + S on the plan of nbits_cases.plan."""
    pieces = 2 * r256(M * 8 * (-(-K // 8)) * 2) + r256(M * 4) if atype == F32 else 0
    splits = plan(M, K, N).splits
    return pieces + (r256(splits * M * N * 4) if splits > 1 else 0)


SHAPES = [(2048, 4096, 4096, 128), (64, 4096, 11008, 128), (2048, 11008, 4096, 128), (17, 4096, 4096, 128), (1, 7, 1, 32), (16, 7, 3, 32),
          (3, 1024, 64, 1024), (5, 1025, 257, 32), (33, 2600, 100, 96), (129, 1088, 130, 1088), (32, 64, 128, 64), (33, 64, 129, 32),
          (128, 8192, 16384, 256), (1, 64, 16385, 32)]


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
@pytest.mark.parametrize("atype", [F32, F16, BF16])
def test_workspace_query_follows_the_stated_formula(lib, shape, atype):
    M, K, N, g = shape
    assert lib.oq_matmul_nbits_fzp_workspace_bytes(M, K, N, g, atype) == stated_formula(M, K, N, atype)
    assert lib.oq_matmul_nbits_fzp_workspace_bytes(M, K, N, g, atype) == lib.oq_matmul_nbits_workspace_bytes(M, K, N, g, atype)


QUERY_CASES = [("M=0", (0, 64, 16, 32, F32)), ("M=-1", (-1, 64, 16, 32, F32)), ("M=2^62", (HUGE, 64, 16, 32, F32)),
               ("K=0", (8, 0, 16, 32, F32)), ("K=2^62", (8, HUGE, 16, 32, F32)), ("N=0", (8, 64, 0, 32, F32)), ("N=2^62", (8, 64, HUGE, 32, F32)),
               ("g=0", (8, 64, 16, 0, F32)), ("g=-1", (8, 64, 16, -1, F32)), ("atype=3", (8, 64, 16, 32, 3)),
               ("N*K>2^40", (1, 1 << 11, 1 << 30, 32, F16)), ("all huge", (HUGE, HUGE, HUGE, HUGE, F32))]


@pytest.mark.parametrize("case", QUERY_CASES, ids=[c[0] for c in QUERY_CASES])
def test_workspace_query_returns_zero_outside_the_bounds(lib, case):
    assert lib.oq_matmul_nbits_fzp_workspace_bytes(*case[1]) == 0
    assert "oq_matmul_nbits_fzp_workspace_bytes" in lib.oq_last_error().decode()
