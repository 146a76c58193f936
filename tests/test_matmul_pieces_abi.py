"""The fp16-piece GEMM of the C ABI (include/oq_hip.h, section N1: oq_matmul_pieces_bytes, oq_matmul_prepare_f32,
oq_matmul_pieces_f32): declared, bound and exported, every refusal answers on the host with its status and a message, and the
size query covers what `matmul_pieces_layout` (csrc/gemm_tn.hip) takes.

Every library call below is one the checks must REFUSE before any device work, so this file is safe on a box with a GPU too:
the pointers are host memory standing in for device memory and nothing may be launched on them."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from piece_gemm_cases import pieces_bytes_at_least

HEADER = os.path.join(ROOT, "include", "oq_hip.h")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
HUGE = (1 << 62) + 12345
TOO_LONG = 8 * 65535 * 4 + 1                      # one row past the 65535 x 4 chunks of the split kernels' grid
NAMES = {"oq_matmul_pieces_bytes": 2, "oq_matmul_prepare_f32": 9, "oq_matmul_pieces_f32": 11}


@pytest.fixture(scope="module")
def lib_path():
    from onnx_quantize_amd import _build
    return _build.build(verbose=False)


@pytest.fixture(scope="module")
def lib(lib_path):
    from onnx_quantize_amd.hip import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def host_ptr():
    buf = (C.c_char * (1 << 18))()
    base = C.addressof(buf)
    yield buf, base + (-base % 256)


def test_the_three_symbols_are_declared_bound_and_exported(lib_path):
    from onnx_quantize_amd.hip import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = C.CDLL(lib_path)
    for name, count in NAMES.items():
        declared = re.findall(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert len(declared) == 1 and len(declared[0].split(",")) == count, (name, declared)
        assert len(_lib.PROTOTYPES[name][1]) == count
        assert hasattr(raw, name), f"{name} is declared in include/oq_hip.h but not exported"
    assert _lib.PROTOTYPES["oq_matmul_pieces_bytes"][0] is C.c_size_t
    assert (_lib.OQ_ERR_INVALID_ARGUMENT, _lib.OQ_ERR_UNSUPPORTED, _lib.OQ_ERR_WORKSPACE) == (INVALID, UNSUPPORTED, WORKSPACE)


# ------------------------------------------------------------------------------------ refusals
def prepare_args(ptr, **over):
    a = dict(X=ptr, Kd=64, cols=16, ldx=64, fast_axis=1, per_row=1, pieces=ptr, pieces_bytes=1 << 17, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


def product_args(ptr, **over):
    a = dict(pieces_a=ptr, pieces_b=ptr + (1 << 17), M=8, N=16, Kd=64, alpha=1.0, beta=0.0, C=ptr, ldc=16, per_row=1, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


NEED_64_16 = 2 * 4 * 2 * 256 * 16 + 16384 + 256         # two stages of pieces, the header, 8 * 16 bytes of row scales in one 256-byte unit
PREPARE_CASES = [
    # (what is hostile, overrides, the status)
    ("null X", dict(X=None), INVALID), ("null pieces", dict(pieces=None), INVALID),
    ("Kd=0", dict(Kd=0), INVALID), ("Kd=-1", dict(Kd=-1), INVALID), ("Kd=2^62", dict(Kd=HUGE, ldx=HUGE), INVALID),
    ("cols=0", dict(cols=0), INVALID), ("cols=-1", dict(cols=-1), INVALID), ("cols=2^62", dict(cols=HUGE), INVALID),
    ("Kd*cols>2^40", dict(Kd=1 << 20, ldx=1 << 20, cols=(1 << 20) + 1), INVALID),
    ("ldx<Kd, fast axis", dict(ldx=63), INVALID), ("ldx<cols, k-major", dict(fast_axis=0, per_row=0, ldx=15), INVALID),
    ("ldx=0", dict(ldx=0), INVALID), ("ldx=2^62", dict(ldx=HUGE), INVALID),
    ("ldx between cols and Kd, fast axis", dict(ldx=16), INVALID),
    ("per-row scales, k-major", dict(fast_axis=0, per_row=1, ldx=16), INVALID),
    ("one byte short", dict(pieces_bytes=NEED_64_16 - 1), WORKSPACE), ("no bytes", dict(pieces_bytes=0), WORKSPACE),
    ("one byte short, k-major", dict(fast_axis=0, per_row=0, ldx=16, pieces_bytes=NEED_64_16 - 1), WORKSPACE),
    ("misaligned pieces", dict(pieces="eight"), WORKSPACE), ("pieces at an odd byte", dict(pieces="odd"), WORKSPACE),
    ("contraction too long", dict(Kd=TOO_LONG, ldx=TOO_LONG, cols=1, pieces_bytes=1 << 62), UNSUPPORTED),
    ("contraction too long, k-major", dict(Kd=TOO_LONG, ldx=1, cols=1, fast_axis=0, per_row=0, pieces_bytes=1 << 62), UNSUPPORTED),
]
PRODUCT_CASES = [
    ("null pieces_a", dict(pieces_a=None), INVALID), ("null pieces_b", dict(pieces_b=None), INVALID), ("null C", dict(C=None), INVALID),
    ("M=0", dict(M=0), INVALID), ("M=-1", dict(M=-1), INVALID), ("M=2^62", dict(M=HUGE), INVALID),
    ("N=0", dict(N=0), INVALID), ("N=-1", dict(N=-1), INVALID), ("N=2^62", dict(N=HUGE, ldc=HUGE), INVALID),
    ("Kd=0", dict(Kd=0), INVALID), ("Kd=-1", dict(Kd=-1), INVALID), ("Kd=2^62", dict(Kd=HUGE), INVALID),
    ("Kd too long", dict(Kd=TOO_LONG, M=1, N=1, ldc=1), INVALID),
    ("ldc<N", dict(ldc=15), INVALID), ("ldc=0", dict(ldc=0), INVALID), ("ldc=2^62", dict(ldc=HUGE), INVALID),
    ("M*ldc>2^40", dict(M=1 << 30, ldc=1 << 11), INVALID),
    ("misaligned pieces_a", dict(pieces_a="eight"), INVALID), ("misaligned pieces_b", dict(pieces_b="eight"), INVALID),
    ("pieces_a at an odd byte", dict(pieces_a="odd", per_row=0), INVALID), ("pieces_b 128-byte aligned", dict(pieces_b="128"), INVALID),
]


def hostile(ptr, over):
    shift = {"odd": 1, "eight": 8, "128": 128}
    return {k: (v if not isinstance(v, str) else ptr + shift[v] if k != "pieces_b" else ptr + (1 << 17) + shift[v]) for k, v in over.items()}


@pytest.mark.parametrize("case", PREPARE_CASES, ids=[c[0] for c in PREPARE_CASES])
def test_prepare_refuses_on_the_host(lib, host_ptr, case):
    buf, ptr = host_ptr
    _, over, status = case
    before = bytes(buf)
    st = lib.oq_matmul_prepare_f32(*prepare_args(ptr, **hostile(ptr, over)))
    msg = lib.oq_last_error().decode()
    assert st == status, (st, msg)
    assert msg and "oq_matmul_prepare_f32" in msg, msg
    assert bytes(buf) == before                                   # nothing written on failure


@pytest.mark.parametrize("case", PRODUCT_CASES, ids=[c[0] for c in PRODUCT_CASES])
def test_the_product_refuses_on_the_host(lib, host_ptr, case):
    buf, ptr = host_ptr
    _, over, status = case
    before = bytes(buf)
    st = lib.oq_matmul_pieces_f32(*product_args(ptr, **hostile(ptr, over)))
    msg = lib.oq_last_error().decode()
    assert st == status, (st, msg)
    assert msg and "oq_matmul_pieces_f32" in msg, msg
    assert bytes(buf) == before


def test_the_refusals_name_what_is_wrong(lib, host_ptr):
    _, ptr = host_ptr
    assert lib.oq_matmul_prepare_f32(*prepare_args(ptr, fast_axis=0, per_row=1, ldx=16)) == INVALID
    assert "per-row scales" in lib.oq_last_error().decode()
    assert lib.oq_matmul_prepare_f32(*prepare_args(ptr, pieces_bytes=NEED_64_16 - 1)) == WORKSPACE
    msg = lib.oq_last_error().decode()
    assert f"{NEED_64_16} bytes" in msg and f"{NEED_64_16 - 1} given" in msg, msg
    assert lib.oq_matmul_prepare_f32(*prepare_args(ptr, Kd=TOO_LONG, ldx=TOO_LONG, cols=1)) == UNSUPPORTED
    assert str(TOO_LONG) in lib.oq_last_error().decode()


# ------------------------------------------------------------------------------------ the size query
def test_the_size_query_returns_zero_outside_the_bounds(lib):
    for Kd, cols in ((0, 7), (7, 0), (-1, 7), (7, -1), (HUGE, 7), (7, HUGE), (HUGE, HUGE), (1 << 31, 1), (1, 1 << 31),
                     (1 << 20, (1 << 20) + 1), (TOO_LONG, 1), (TOO_LONG, 256)):
        assert lib.oq_matmul_pieces_bytes(Kd, cols) == 0, (Kd, cols)
    assert lib.oq_matmul_pieces_bytes(TOO_LONG - 1, 1) != 0 and lib.oq_matmul_pieces_bytes(1 << 20, 1 << 20) != 0


def test_the_size_query_is_monotone_and_covers_the_layout(lib):
    values = [1, 7, 8, 9, 31, 32, 33, 64, 100, 255, 256, 257, 512, 513, 1000, 2081]
    grid = [[lib.oq_matmul_pieces_bytes(Kd, cols) for cols in values] for Kd in values]
    for i, Kd in enumerate(values):
        for j, cols in enumerate(values):
            need = grid[i][j]
            assert need >= pieces_bytes_at_least(Kd, cols) and need % 256 == 0, (Kd, cols, need)
            assert need < pieces_bytes_at_least(Kd, cols) + 256, (Kd, cols, need)                   # nothing but the rounding of the last piece
            assert i == 0 or need >= grid[i - 1][j], (Kd, cols)
            assert j == 0 or need >= grid[i][j - 1], (Kd, cols)
    assert lib.oq_matmul_pieces_bytes(64, 16) == NEED_64_16
    assert grid[values.index(33)][0] > grid[values.index(32)][0] and grid[0][values.index(257)] > grid[0][values.index(256)]
