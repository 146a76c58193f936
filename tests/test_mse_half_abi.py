"""oq_rtn_mse_h16 and oq_rtn_mse_half_workspace_bytes (include/oq_hip_half.h): declared, bound and exported, plain C99, and their
argument checks answer without a GPU.  Also here, on the CPU: the share of rows the oracle case of tests/test_mse_half_gpu.py
leaves undecided, which depends on the input and the oracle alone.

Every call of the sweep below is one the checks must REFUSE before any device call, so this file is safe on a box with a GPU
too: the pointers are host memory standing in for device memory and nothing may be launched on them."""
import ctypes as C
import os
import re
import subprocess

import pytest

import mse_half_cases as M
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "oq_hip_half.h")
NAME, QUERY = "oq_rtn_mse_h16", "oq_rtn_mse_half_workspace_bytes"


@pytest.fixture(scope="module")
def lib_path():
    from onnx_quantize_amd import _build
    return _build.build(verbose=False)


@pytest.fixture(scope="module")
def lib(lib_path):
    from onnx_quantize_amd.hip import _lib
    return _lib.load()


def test_the_entry_points_are_declared_bound_and_exported(lib_path):
    from onnx_quantize_amd.hip import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint32_t\s+%s\s*\(" % NAME, text) and re.search(r"\bsize_t\s+%s\s*\(" % QUERY, text)
    raw = C.CDLL(lib_path)
    for name in (NAME, QUERY):
        assert name in _lib.HALF_PROTOTYPES and name not in _lib.PROTOTYPES
        assert hasattr(raw, name), f"{name} is not exported by the library"
    # the signatures of the calls they stand next to: oq_rtn_quantize_h16 and its workspace query
    assert _lib.HALF_PROTOTYPES[NAME] == _lib.HALF_PROTOTYPES["oq_rtn_quantize_h16"]
    assert _lib.HALF_PROTOTYPES[QUERY] == _lib.HALF_PROTOTYPES["oq_rtn_half_workspace_bytes"]
    assert _lib.OQ_ABI_VERSION == 2 and _lib.OQ_HALF_EXTENSION_VERSION == 1 == raw.oq_half_extension_version()     # additions only


def test_half_header_is_plain_c99_with_the_new_names_taken(tmp_path):
    src = tmp_path / "mse_half_header.c"
    src.write_text('#include "oq_hip_half.h"\n'
                   "typedef void (*fn)(void);\n"
                   "fn taken[] = {(fn)oq_rtn_mse_h16, (fn)oq_rtn_mse_half_workspace_bytes, (fn)oq_rtn_quantize_h16};\n"
                   "int codes[] = {OQ_W_F16, OQ_W_BF16, OQ_HALF_EXTENSION_VERSION, OQ_LAYOUT_KN};\n")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                         str(tmp_path / "mse_half_header.o")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr


# ------------------------------------------------------------------------------------ hostile arguments
F16, BF16, TENSOR, CHANNEL, GROUP, UINT4, KN, NBITS, PACKED4 = 0, 1, 0, 1, 2, 1, 0, 1, 2
HUGE = (1 << 62) + 12345


@pytest.fixture(scope="module")
def host_ptr():
    buf = (C.c_char * (1 << 20))()
    base = C.addressof(buf)
    yield buf, base + (-base % 16)


def mse_args(ptr, **over):
    a = dict(W=ptr, wtype=F16, K=256, N=64, ldw=64, qtype=UINT4, strategy=GROUP, group_size=128, symmetric=0, reduce_range=0,
             clip_ratio=1.0, q_out=ptr, scale_out=ptr, zp_out=ptr, layout=KN, workspace=ptr, workspace_bytes=1 << 19, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


def test_the_codes_used_here_are_the_library_s():
    from onnx_quantize_amd.hip import _lib as L
    assert (L.OQ_W_F16, L.OQ_W_BF16, L.OQ_GROUP, L.OQ_UINT4) == (F16, BF16, GROUP, UINT4)
    assert (L.STRATEGY_CODE["tensor"], L.STRATEGY_CODE["channel"], L.STRATEGY_CODE["group"]) == (TENSOR, CHANNEL, GROUP)
    assert (L.OQ_LAYOUT_KN, L.OQ_LAYOUT_NBITS, L.OQ_LAYOUT_KN_PACKED4) == (KN, NBITS, PACKED4)


CASES = [
    # (what is hostile, overrides, statuses allowed, a word of the message that names the argument, the entry point is named)
    ("null W", dict(W=None), (-1,), "null W", True), ("null scale", dict(scale_out=None), (-1,), "scale_out", True),
    ("null zp", dict(zp_out=None), (-1,), "zp_out", True),
    ("wtype=2", dict(wtype=2), (-1,), "wtype 2", True), ("wtype=-1", dict(wtype=-1), (-1,), "wtype -1", True),
    ("odd W", dict(W=1), (-1,), "2-byte aligned", True), ("scale_out + 2", dict(scale_out=2), (-1,), "4-byte aligned", True),
    ("K=0", dict(K=0), (-1,), "K=0", True), ("K=-1", dict(K=-1), (-1,), "K=-1", True), ("K=2^62", dict(K=HUGE), (-1, -2), "K=", True),
    ("N=0", dict(N=0), (-1,), "N=0", True), ("N=-1", dict(N=-1), (-1,), "N=-1", True),
    ("N=2^62", dict(N=HUGE, ldw=HUGE), (-1, -2), "N=", True),
    ("ldw=2^62", dict(ldw=HUGE), (-1, -2), "ldw=", True), ("ldw<N", dict(ldw=63), (-1,), "ldw=63", True),
    ("all huge", dict(K=HUGE, N=HUGE, ldw=HUGE, group_size=HUGE, workspace_bytes=1 << 62), (-1, -2), "K=", True),
    ("2^31 x 2^31", dict(K=(1 << 31) - 1, N=(1 << 31) - 1, ldw=(1 << 31) - 1), (-2,), "too large", True),
    ("groups beyond the grid", dict(K=1 << 20, N=4, ldw=4, group_size=16), (-2,), "65535 groups", True),
    ("clip 0", dict(clip_ratio=0.0), (-1,), "clip_ratio", False), ("clip 1.5", dict(clip_ratio=1.5), (-1,), "clip_ratio", False),
    ("clip nan", dict(clip_ratio=float("nan")), (-1,), "clip_ratio", False),
    ("qtype", dict(qtype=99), (-1,), "quantization type", False), ("qtype 32 bit", dict(qtype=4), (-2,), "32-bit", False),
    ("strategy", dict(strategy=9), (-1,), "strategy", False),
    ("group_size=0", dict(group_size=0), (-1,), "group_size", False), ("group_size=-5", dict(group_size=-5), (-1,), "group_size", False),
    ("straddling groups", dict(group_size=96), (-2,), "group_size 96", True),
    ("layout", dict(layout=9), (-1,), "layout 9", True),
    ("layout nbits", dict(layout=NBITS), (-2,), "NBITS", True), ("layout packed4", dict(layout=PACKED4), (-2,), "KN_PACKED4", True),
    ("no workspace", dict(workspace=None), (-3,), "workspace", True), ("short workspace", dict(workspace_bytes=64), (-3,), "workspace", True),
    ("workspace + 2", dict(workspace=2), (-3,), "4-byte aligned", True),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_mse_h16_refuses_hostile_arguments(lib, host_ptr, case):
    _, ptr = host_ptr
    _, over, allowed, word, named = case
    for key in ("W", "scale_out", "workspace"):                         # an integer stands for "the buffer plus that many bytes"
        if isinstance(over.get(key), int):
            over = dict(over, **{key: ptr + over[key]})
    for wtype in ((F16, BF16) if "wtype" not in over else (over["wtype"],)):
        st = lib.oq_rtn_mse_h16(*mse_args(ptr, **dict(over, wtype=wtype)))
        msg = lib.oq_last_error().decode()
        assert st in allowed, (st, msg)
        assert word in msg and (NAME in msg or not named), msg


def test_a_short_workspace_names_the_need(lib, host_ptr):
    _, ptr = host_ptr
    need = lib.oq_rtn_mse_half_workspace_bytes(256, 64, GROUP, 128)
    assert need == 2 * 64 * 12 + 1024 * 20 * 4 + 512                      # a 12-byte row per (scale, zp) pair + the tensor partials + the head
    st = lib.oq_rtn_mse_h16(*mse_args(ptr, workspace_bytes=need - 1))
    assert st == -3 and str(need) in lib.oq_last_error().decode()


@pytest.mark.parametrize("strategy,g", [(GROUP, 16), (GROUP, 32), (GROUP, 64), (GROUP, 128), (GROUP, 256), (GROUP, 512), (GROUP, -1),
                                        (GROUP, 1 << 20), (CHANNEL, -1), (TENSOR, -1)])
def test_the_workspace_query_is_the_mse_part_of_the_fp32_query(lib, strategy, g):
    """oq_rtn_workspace_bytes(mse = 1) - oq_rtn_workspace_bytes(mse = 0) is what the search itself needs: the same formula."""
    for k, n in ((512, 1), (512, 520), (1024, 257), (4096, 11008), (33, 72)):
        if strategy == GROUP and g > 0 and k % min(g, k):
            continue
        f32 = lib.oq_rtn_workspace_bytes(k, n, strategy, g, 1) - lib.oq_rtn_workspace_bytes(k, n, strategy, g, 0)
        got = lib.oq_rtn_mse_half_workspace_bytes(k, n, strategy, g)
        assert got == f32 > 0, (k, n, strategy, g, got, f32)


QUERY_CASES = [("K=0", (0, 64, GROUP, 128), "K=0"), ("K=-1", (-1, 64, GROUP, 128), "K=-1"), ("K=2^62", (HUGE, 64, GROUP, 128), "K="),
               ("N=0", (256, 0, GROUP, 128), "N=0"), ("N=-1", (256, -1, CHANNEL, -1), "N=-1"), ("N=2^62", (256, HUGE, CHANNEL, -1), "N="),
               ("all huge", (HUGE, HUGE, GROUP, HUGE), "K="), ("strategy", (256, 64, 9, 128), "strategy"),
               ("group_size=0", (256, 64, GROUP, 0), "group_size"), ("straddling", (256, 64, GROUP, 96), "straddle")]


@pytest.mark.parametrize("case", QUERY_CASES, ids=[c[0] for c in QUERY_CASES])
def test_the_workspace_query_refuses_hostile_arguments(lib, case):
    _, args, word = case
    assert lib.oq_rtn_mse_half_workspace_bytes(*args) == 0
    assert word in lib.oq_last_error().decode()


# ------------------------------------------------------------------------------------ the oracle case's input, on the CPU
@pytest.mark.parametrize("g", M.ORACLE_GROUPS)
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_the_oracle_case_leaves_at_most_one_percent_of_its_rows_undecided(dtype, g):
    """The GPU test caps the undecided share at 1 %; that share is a property of the input and the oracle, fixed here so that
    the cap cannot hide a kernel error."""
    w = M.oracle_matrix(dtype)
    assert w.shape == M.ORACLE_SHAPE and w.dtype.name == "float32" and (M.round_to(w, dtype) == w).all()
    undecided, rows, _, j = M.undecided_rows(w, g)
    assert rows == w.size // g
    assert undecided <= rows // 100, (dtype, g, undecided, rows)
    assert j.stop_decided
