"""The decode extension of the C ABI (include/oq_hip_nbits_decode.h): declared, bound and exported as one set, plain C99, its
refusals answer on the host with their status and a message, and its workspace query follows the formula the header states.
oq_hip.h, oq_hip_half.h and oq_hip_nbits.h keep their pins.

Every library call below is one the checks must REFUSE before any device work, so this file is safe on a box with a GPU too:
the pointers are host memory standing in for device memory and nothing may be launched on them."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "oq_hip_nbits_decode.h")
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
    assert declared_symbols(HEADER) == sorted(_lib.NBITS_DECODE_PROTOTYPES)
    others = set(_lib.PROTOTYPES) | set(_lib.HALF_PROTOTYPES) | set(_lib.NBITS_PROTOTYPES) | set(_lib.QLINEAR_PROTOTYPES)
    assert not set(_lib.NBITS_DECODE_PROTOTYPES) & others
    raw = C.CDLL(lib_path)
    for name in _lib.NBITS_DECODE_PROTOTYPES:
        assert hasattr(raw, name), f"{name} is declared in include/oq_hip_nbits_decode.h but not exported"
    assert len(_lib.NBITS_DECODE_PROTOTYPES["oq_matmul_nbits_decode"][1]) == 20          # oq_matmul_nbits' 19 and zero_points_type
    assert len(_lib.NBITS_DECODE_PROTOTYPES["oq_matmul_nbits_decode_workspace_bytes"][1]) == 5
    assert raw.oq_nbits_decode_extension_version() == 1 == _lib.OQ_NBITS_DECODE_EXTENSION_VERSION
    assert _lib.OQ_NBITS_ZP_PACKED_U8 == ZP_U8
    assert raw.oq_abi_version() == 2 and raw.oq_half_extension_version() == 1 and raw.oq_nbits_extension_version() == 1      # the pins stay


def test_the_header_is_plain_c99(tmp_path):
    src = tmp_path / "nbits_decode_header.c"
    src.write_text('#include "oq_hip_nbits_decode.h"\n'
                   "typedef void (*fn)(void);\n"
                   "fn taken[] = {(fn)oq_nbits_decode_extension_version, (fn)oq_matmul_nbits_decode_workspace_bytes, (fn)oq_matmul_nbits_decode,\n"
                   "              (fn)oq_matmul_nbits};\n"
                   "int codes[] = {OQ_NBITS_F32, OQ_NBITS_F16, OQ_NBITS_BF16, OQ_NBITS_ZP_PACKED_U8, OQ_NBITS_DECODE_EXTENSION_VERSION,\n"
                   "               OQ_NBITS_EXTENSION_VERSION, OQ_NBITS_G_IDX, OQ_ERR_UNSUPPORTED};\n")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                         str(tmp_path / "nbits_decode_header.o")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr


# ------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def host_ptr():
    buf = (C.c_char * (1 << 18))()
    base = C.addressof(buf)
    yield buf, base + (-base % 256)


def call_args(ptr, **over):
    a = dict(A=ptr, atype=F32, M=8, K=2048, lda=2048, B=ptr, bits=4, N=16, group_size=32, scales=ptr, scales_type=F32, zero_points=None,
             zero_points_type=ZP_U8, bias=None, flags=0, Y=ptr, ldy=16, workspace=ptr, workspace_bytes=1 << 17, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
CASES = [
    # (what is hostile, overrides, status, a word of the message)
    ("null A", dict(A=None), INVALID, "null"), ("null B", dict(B=None), INVALID, "null"),
    ("null scales", dict(scales=None), INVALID, "null"), ("null Y", dict(Y=None), INVALID, "null"),
    ("atype=3", dict(atype=3), INVALID, "atype"), ("atype=-1", dict(atype=-1), INVALID, "atype"),
    ("fp16 scales for fp32 A", dict(scales_type=F16), INVALID, "scales_type"), ("scales_type=9", dict(scales_type=9), INVALID, "scales_type"),
    ("fp16 zero points for fp32 A", dict(zero_points="ptr", zero_points_type=F16), INVALID, "zero_points_type"),
    ("zero_points_type=7", dict(zero_points_type=7), INVALID, "zero_points_type"),
    ("float flag on packed zero points", dict(zero_points="ptr", flags=1), INVALID, "flags"),
    ("M=0", dict(M=0), INVALID, "M=0"), ("M=-1", dict(M=-1), INVALID, "M=-1"), ("M=2^62", dict(M=HUGE), INVALID, "M="),
    ("K=0", dict(K=0), INVALID, "K=0"), ("K=-1", dict(K=-1), INVALID, "K=-1"), ("K=2^62", dict(K=HUGE, lda=HUGE), INVALID, "K="),
    ("N=0", dict(N=0), INVALID, "N=0"), ("N=-1", dict(N=-1), INVALID, "N=-1"), ("N=2^62", dict(N=HUGE, ldy=HUGE), INVALID, "N="),
    ("lda<K", dict(lda=2047), INVALID, "lda=2047"), ("lda=2^62", dict(lda=HUGE), INVALID, "lda="),
    ("ldy<N", dict(ldy=15), INVALID, "ldy=15"), ("ldy=2^62", dict(ldy=HUGE), INVALID, "ldy="),
    ("N*K>2^40", dict(N=1 << 30, ldy=1 << 30, K=1 << 11, lda=1 << 11, M=1), INVALID, "2^40"),
    ("all huge", dict(M=HUGE, K=HUGE, N=HUGE, lda=HUGE, ldy=HUGE, group_size=HUGE, workspace_bytes=1 << 62), INVALID, "M="),
    ("M=17", dict(M=17), UNSUPPORTED, "M = 17"), ("M=2048", dict(M=2048), UNSUPPORTED, "M = 2048"),
    ("bits=2", dict(bits=2), UNSUPPORTED, "bits = 2"), ("bits=16", dict(bits=16), UNSUPPORTED, "bits = 16"),
    ("g=24", dict(group_size=24), UNSUPPORTED, "group_size = 24"), ("g=8", dict(group_size=8), UNSUPPORTED, "group_size = 8"),
    ("g=0", dict(group_size=0), UNSUPPORTED, "group_size = 0"), ("g=-16", dict(group_size=-16), UNSUPPORTED, "group_size"),
    ("g_idx", dict(flags=2), UNSUPPORTED, "g_idx"), ("unknown flag", dict(flags=8), INVALID, "flags"),
    ("odd A", dict(A="odd"), INVALID, "aligned"), ("odd Y", dict(Y="odd"), INVALID, "aligned"),
    ("odd scales", dict(scales="odd"), INVALID, "aligned"), ("odd bias", dict(bias="odd"), INVALID, "aligned"),
    ("odd float zero points", dict(zero_points="odd", zero_points_type=F32), INVALID, "aligned"),
    ("B off by 8", dict(B="eight"), INVALID, "16-byte"),
    ("null workspace", dict(workspace=None), WORKSPACE, "workspace"), ("short workspace", dict(workspace_bytes=64), WORKSPACE, "workspace"),
    ("workspace one byte short", dict(workspace_bytes=2 * 8 * 16 * 4 - 1), WORKSPACE, "workspace"),
    ("misaligned workspace", dict(workspace="eight"), WORKSPACE, "workspace"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_matmul_nbits_decode_refuses_on_the_host(lib, host_ptr, case):
    buf, ptr = host_ptr
    _, over, expected, word = case
    over = {k: (ptr + 1 if v == "odd" else ptr + 8 if v == "eight" else ptr if v == "ptr" else v) for k, v in over.items()}
    before = bytes(buf)
    st = lib.oq_matmul_nbits_decode(*call_args(ptr, **over))
    msg = lib.oq_last_error().decode()
    assert st == expected, (st, msg)
    assert word in msg, msg
    assert bytes(buf) == before                                   # nothing written on failure


def test_what_the_tile_kernel_refuses_passes_the_host_checks_up_to_the_workspace(lib, host_ptr):
    """group_size 16 and float zero points are no refusals here: with everything else in order the call gets as far as the
    workspace check, the last one before the launch."""
    _, ptr = host_ptr
    for over in (dict(group_size=16), dict(zero_points=ptr, zero_points_type=F32), dict(zero_points=ptr, zero_points_type=F32, flags=1)):
        st = lib.oq_matmul_nbits_decode(*call_args(ptr, workspace=None, **over))
        assert st == WORKSPACE, (over, st, lib.oq_last_error().decode())


# ------------------------------------------------------------------------------------ the workspace query
def r256(n):
    return (n + 255) // 256 * 256


def stated_formula(M, K, N):
    """include/oq_hip_nbits_decode.h, `workspace`."""
    splits = -(-K // 1024)
    return r256(splits * M * N * 4) if splits > 1 else 0


SHAPES = [(1, 4096, 4096, 128), (16, 4096, 4096, 128), (1, 4096, 11008, 128), (16, 4096, 11008, 128), (1, 11008, 4096, 128), (16, 11008, 4096, 16),
          (1, 7, 1, 16), (16, 7, 3, 16), (3, 1024, 64, 1024), (5, 1025, 257, 32), (9, 2600, 100, 48), (16, 1088, 130, 1088), (2, 16, 2, 16)]


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
@pytest.mark.parametrize("atype", [F32, F16, BF16])
def test_workspace_query_follows_the_stated_formula(lib, shape, atype):
    M, K, N, g = shape
    assert lib.oq_matmul_nbits_decode_workspace_bytes(M, K, N, g, atype) == stated_formula(M, K, N)


def test_one_slice_needs_no_workspace_and_model_sizes_need_their_slabs(lib):
    assert lib.oq_matmul_nbits_decode_workspace_bytes(16, 1024, 4096, 128, F16) == 0
    assert lib.oq_matmul_nbits_decode_workspace_bytes(16, 11008, 4096, 128, F16) == 11 * 16 * 4096 * 4


QUERY_CASES = [("M=0", (0, 64, 16, 32, F32)), ("M=-1", (-1, 64, 16, 32, F32)), ("M=17", (17, 64, 16, 32, F32)), ("M=2^62", (HUGE, 64, 16, 32, F32)),
               ("K=0", (8, 0, 16, 32, F32)), ("K=2^62", (8, HUGE, 16, 32, F32)), ("N=0", (8, 64, 0, 32, F32)), ("N=2^62", (8, 64, HUGE, 32, F32)),
               ("g=0", (8, 64, 16, 0, F32)), ("g=-1", (8, 64, 16, -1, F32)), ("g=24", (8, 64, 16, 24, F32)), ("atype=3", (8, 64, 16, 32, 3)),
               ("N*K>2^40", (1, 1 << 11, 1 << 30, 32, F16)), ("all huge", (HUGE, HUGE, HUGE, HUGE, F32))]


@pytest.mark.parametrize("case", QUERY_CASES, ids=[c[0] for c in QUERY_CASES])
def test_workspace_query_returns_zero_outside_the_bounds(lib, case):
    assert lib.oq_matmul_nbits_decode_workspace_bytes(*case[1]) == 0
