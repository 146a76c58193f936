"""The GPTQ row loop of the C ABI (include/oq_hip.h: oq_gptq_loop_workspace_bytes, oq_gptq_loop_f32): declared, bound and exported,
every refusal answers on the host with its status and a word of its message, and the size query returns 0 outside the bounds.

Every library call below is one the checks must REFUSE before any device work, so this file is safe on a box with a GPU too: the
pointers are host memory standing in for device memory and nothing may be launched on them."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "oq_hip.h")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
HUGE = (1 << 62) + 12345
MAX_EXTENT = (1 << 31) - 1
MAX_K = 1 << 17
INT4, UINT4, INT8, UINT8, INT32 = 0, 1, 2, 3, 4
KN, NBITS, PACKED4 = 0, 1, 2
NAMES = {"oq_gptq_loop_workspace_bytes": 3, "oq_gptq_loop_f32": 24}
K, N = 64, 16


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


def test_the_two_symbols_are_declared_bound_and_exported(lib_path):
    from onnx_quantize_amd.hip import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = C.CDLL(lib_path)
    for name, count in NAMES.items():
        declared = re.findall(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert len(declared) == 1 and len(declared[0].split(",")) == count, (name, declared)
        assert len(_lib.PROTOTYPES[name][1]) == count
        assert hasattr(raw, name), f"{name} is declared in include/oq_hip.h but not exported"
    assert _lib.PROTOTYPES["oq_gptq_loop_workspace_bytes"][0] is C.c_size_t
    assert (_lib.OQ_ERR_INVALID_ARGUMENT, _lib.OQ_ERR_UNSUPPORTED, _lib.OQ_ERR_WORKSPACE) == (INVALID, UNSUPPORTED, WORKSPACE)
    assert (_lib.OQ_INT4, _lib.OQ_UINT4, _lib.OQ_INT8, _lib.OQ_UINT8, _lib.OQ_INT32) == (INT4, UINT4, INT8, UINT8, INT32)
    assert (_lib.OQ_LAYOUT_KN, _lib.OQ_LAYOUT_NBITS, _lib.OQ_LAYOUT_KN_PACKED4) == (KN, NBITS, PACKED4)
    assert (_lib.OQ_GPTQ_PARITY, _lib.OQ_GPTQ_CORRECTED, _lib.OQ_GPTQ_CORRECTED_COLUMNS) == (0, 1, 2)


def loop_args(lib, ptr, **over):
    """A call that would run (group parameters, corrected mode, a workspace of the queried size) but for the overrides."""
    a = dict(W=ptr, K=K, N=N, U=ptr + 4096, qtype=INT8, group_size=32, symmetric=0, reduce_range=0, clip_ratio=1.0, mse=0, block_size=128,
             mode=1, method=0, init_scale=ptr + 32768, init_zp=ptr + 36864, init_count=N, q_int_out=ptr + 40960, q_layout=KN,
             q_deq_out=ptr + 45056, used_scale=ptr + 49152, used_zp=ptr + 53248, workspace=ptr + 65536, workspace_bytes=None, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(lib.oq_gptq_loop_workspace_bytes(K, N, 128), 1 << 20)
    if a["workspace_bytes"] < 0:                                        # so many bytes short of the query
        a["workspace_bytes"] += lib.oq_gptq_loop_workspace_bytes(a["K"], a["N"], a["block_size"])
    return list(a.values())


CASES = [
    # (what is hostile, overrides, the status, a word of the message)
    ("null W", dict(W=None), INVALID, "bad argument"), ("null U", dict(U=None), INVALID, "bad argument"),
    ("null init_scale", dict(init_scale=None), INVALID, "bad argument"), ("null init_zp", dict(init_zp=None), INVALID, "bad argument"),
    ("null q_int_out", dict(q_int_out=None), INVALID, "bad argument"), ("null q_deq_out", dict(q_deq_out=None), INVALID, "bad argument"),
    ("K=0", dict(K=0), INVALID, "bad argument"), ("K=-1", dict(K=-1), INVALID, "bad argument"),
    ("N=0", dict(N=0, init_count=1), INVALID, "bad argument"), ("N=-1", dict(N=-1, init_count=1), INVALID, "bad argument"),
    ("K=2^17+1", dict(K=MAX_K + 1), UNSUPPORTED, "too large"), ("K=2^62", dict(K=HUGE), UNSUPPORTED, "too large"),
    ("N=2^31", dict(N=1 << 31, init_count=1), UNSUPPORTED, "too large"), ("N=2^62", dict(N=HUGE, init_count=1), UNSUPPORTED, "too large"),
    ("K*N>2^40", dict(K=MAX_K, N=(1 << 23) + 1, init_count=1), UNSUPPORTED, "too large"),
    ("init_count=0", dict(init_count=0), INVALID, "init_count"), ("init_count=2", dict(init_count=2), INVALID, "init_count"),
    ("init_count=N-1", dict(init_count=N - 1), INVALID, "init_count"), ("init_count=N+1", dict(init_count=N + 1), INVALID, "init_count"),
    ("init_count=-1", dict(init_count=-1), INVALID, "init_count"),
    ("block_size=0", dict(block_size=0), INVALID, "block_size"), ("block_size=-1", dict(block_size=-1), INVALID, "block_size"),
    ("block_size=2^31", dict(block_size=1 << 31), INVALID, "block_size"), ("group_size=2^31", dict(group_size=1 << 31), INVALID, "block_size"),
    ("mode=3", dict(mode=3), INVALID, "bad mode 3"), ("mode=-1", dict(mode=-1), INVALID, "bad mode -1"),
    ("method=5", dict(method=5), INVALID, "unknown method 5"), ("method=-1", dict(method=-1), INVALID, "unknown method -1"),
    ("q_layout=nbits", dict(q_layout=NBITS), INVALID, "bad q_layout 1"), ("q_layout=3", dict(q_layout=3), INVALID, "bad q_layout 3"),
    ("q_layout=-1", dict(q_layout=-1), INVALID, "bad q_layout -1"),
    ("packed int8", dict(q_layout=PACKED4, qtype=INT8), UNSUPPORTED, "packed layout"),
    ("packed uint8", dict(q_layout=PACKED4, qtype=UINT8), UNSUPPORTED, "packed layout"),
    ("packed odd N", dict(q_layout=PACKED4, qtype=UINT4, N=15, init_count=15), UNSUPPORTED, "even N"),
    ("packed int4 N=1", dict(q_layout=PACKED4, qtype=INT4, N=1, init_count=1), UNSUPPORTED, "even N"),
    ("clip_ratio=0", dict(clip_ratio=0.0), INVALID, "clip_ratio"), ("clip_ratio=-0.5", dict(clip_ratio=-0.5), INVALID, "clip_ratio"),
    ("clip_ratio=1.5", dict(clip_ratio=1.5), INVALID, "clip_ratio"), ("clip_ratio=nan", dict(clip_ratio=float("nan")), INVALID, "clip_ratio"),
    ("qtype=6", dict(qtype=6), INVALID, "unknown quantization type"), ("qtype=-1", dict(qtype=-1), INVALID, "unknown quantization type"),
    ("qtype=int32", dict(qtype=INT32), UNSUPPORTED, "32-bit"),
    ("used_scale without used_zp", dict(used_zp=None), INVALID, "used_zp missing"),
    ("one byte short", dict(workspace_bytes=-1), WORKSPACE, "workspace"), ("no bytes", dict(workspace_bytes=0), WORKSPACE, "workspace"),
    ("one byte short, tall block", dict(workspace_bytes=-1, block_size=256, K=300), WORKSPACE, "workspace"),
    ("one byte short, parity", dict(workspace_bytes=-1, mode=0), WORKSPACE, "workspace"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_loop_refuses_on_the_host(lib, host_ptr, case):
    buf, ptr = host_ptr
    _, over, status, word = case
    before = bytes(buf)
    st = lib.oq_gptq_loop_f32(*loop_args(lib, ptr, **over))
    msg = lib.oq_last_error().decode()
    assert st == status, (st, msg)
    assert msg and word in msg, msg
    assert bytes(buf) == before                                   # nothing written on failure


def test_the_workspace_refusal_names_both_sizes(lib, host_ptr):
    _, ptr = host_ptr
    need = lib.oq_gptq_loop_workspace_bytes(K, N, 128)
    assert need > 0
    assert lib.oq_gptq_loop_f32(*loop_args(lib, ptr, workspace_bytes=need - 1)) == WORKSPACE
    msg = lib.oq_last_error().decode()
    assert "oq_gptq_loop_f32" in msg and f"{need} bytes needed" in msg and f"{need - 1} given" in msg, msg


def test_the_size_query_returns_zero_outside_the_bounds(lib):
    q = lib.oq_gptq_loop_workspace_bytes
    for k, n, bs in ((0, 7, 128), (7, 0, 128), (-1, 7, 128), (7, -1, 128), (HUGE, 7, 128), (7, HUGE, 128), (MAX_K + 1, 7, 128),
                     (7, 1 << 31, 128), (MAX_K, (1 << 23) + 1, 128), (64, 16, 0), (64, 16, -1), (64, 16, 1 << 31), (64, 16, HUGE)):
        assert q(k, n, bs) == 0, (k, n, bs)
    assert q(MAX_K, 1, 128) != 0 and q(1, MAX_EXTENT, 128) != 0 and q(MAX_K, 1 << 23, 128) != 0 and q(64, 16, MAX_EXTENT) != 0
    assert q(1, 1, 1) != 0


def test_the_size_query_grows_with_its_arguments(lib):
    q = lib.oq_gptq_loop_workspace_bytes
    values = [1, 15, 16, 17, 127, 128, 129, 512, 513, 1100]
    for bs in (18, 128, 320):
        grid = [[q(k, n, bs) for n in values] for k in values]
        for i in range(len(values)):
            for j in range(len(values)):
                assert grid[i][j] > 0
                assert i == 0 or grid[i][j] >= grid[i - 1][j], (values[i], values[j], bs)
                assert j == 0 or grid[i][j] >= grid[i][j - 1], (values[i], values[j], bs)
    assert q(600, 64, 256) > q(600, 64, 128)                       # a tall block's working copy
