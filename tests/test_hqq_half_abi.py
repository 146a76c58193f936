"""oq_hqq_optimize_h16 (include/oq_hip_half.h): declared, bound and exported, plain C99, and its argument checks answer
without a GPU.

Every call of the sweep below is one the checks must REFUSE before any device call, so this file is safe on a box with a GPU
too: the pointers are host memory standing in for device memory and nothing may be launched on them."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "oq_hip_half.h")
NAME = "oq_hqq_optimize_h16"


@pytest.fixture(scope="module")
def lib_path():
    from onnx_quantize_amd import _build
    return _build.build(verbose=False)


@pytest.fixture(scope="module")
def lib(lib_path):
    from onnx_quantize_amd.hip import _lib
    return _lib.load()


def test_the_entry_point_is_declared_bound_and_exported(lib_path):
    from onnx_quantize_amd.hip import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint32_t\s+%s\s*\(" % NAME, text)
    assert NAME in _lib.HALF_PROTOTYPES and NAME not in _lib.PROTOTYPES
    f32 = _lib.PROTOTYPES["oq_hqq_optimize_f32"]
    res, args = _lib.HALF_PROTOTYPES[NAME]
    assert res is f32[0] and args == [f32[1][0], C.c_int32, *f32[1][1:]]          # the fp32 signature with `wtype` behind W
    assert hasattr(C.CDLL(lib_path), NAME)
    assert _lib.OQ_ABI_VERSION == 2 and _lib.OQ_HALF_EXTENSION_VERSION == 1


def test_half_header_is_plain_c99_with_the_new_name_taken(tmp_path):
    src = tmp_path / "hqq_half_header.c"
    src.write_text('#include "oq_hip_half.h"\n'
                   "typedef void (*fn)(void);\n"
                   "fn taken[] = {(fn)oq_hqq_optimize_h16, (fn)oq_hqq_optimize_f32, (fn)oq_hqq_workspace_bytes};\n"
                   "int codes[] = {OQ_W_F16, OQ_W_BF16, OQ_HALF_EXTENSION_VERSION, OQ_ABI_VERSION};\n")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                         str(tmp_path / "hqq_half_header.o")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr


# ------------------------------------------------------------------------------------ hostile arguments
F16, BF16, KN, NBITS = 0, 1, 0, 1
HUGE = (1 << 62) + 12345


@pytest.fixture(scope="module")
def host_ptr():
    buf = (C.c_char * (1 << 20))()
    base = C.addressof(buf)
    yield buf, base + (-base % 16)


def optimize_args(ptr, **over):
    a = dict(W=ptr, wtype=F16, K=128, N=64, ldw=64, group_size=64, reduce_range=0, scale=ptr, zero_point_in=ptr, lp_norm=0.7,
             beta=10.0, kappa=1.01, iters=20, early_stop=1, per_round_launches=0, q_out=ptr, layout=KN, zero_point_out=ptr,
             rounds_out=ptr, workspace=ptr, workspace_bytes=1 << 19, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


CASES = [
    # (what is hostile, overrides, statuses allowed, a word of the message that names the argument)
    ("wtype=2", dict(wtype=2), (-1,), "wtype 2"), ("wtype=-1", dict(wtype=-1), (-1,), "wtype -1"),
    ("K=0", dict(K=0), (-1,), "K=0"), ("K=-1", dict(K=-1), (-1,), "K=-1"), ("K=2^62", dict(K=HUGE), (-1,), "K="),
    ("N=0", dict(N=0), (-1,), "N=0"), ("N=-1", dict(N=-1), (-1,), "N=-1"), ("N=2^62", dict(N=HUGE, ldw=HUGE), (-1,), "N="),
    ("ldw=0", dict(ldw=0), (-1,), "ldw=0"), ("ldw=-1", dict(ldw=-1), (-1,), "ldw=-1"), ("ldw=2^62", dict(ldw=HUGE), (-1,), "ldw="),
    ("ldw<N", dict(ldw=63), (-1,), "ldw=63"),
    ("group_size=0", dict(group_size=0), (-1,), "group_size 0"),
    ("straddling groups", dict(K=96, group_size=64), (-2,), "group_size 64"),
    ("iters=-1", dict(iters=-1), (-1,), "iters=-1"), ("beta=0", dict(beta=0.0), (-1,), "beta=0"),
    ("layout", dict(layout=9), (-1,), "layout 9"), ("layout packed4", dict(layout=2), (-1,), "layout 2"),
    ("null W", dict(W=None), (-1,), "null W"), ("null scale", dict(scale=None), (-1,), "null scale"),
    ("null zero_point_in", dict(zero_point_in=None), (-1,), "null zero_point_in"),
    ("null zero_point_out", dict(zero_point_out=None), (-1,), "null zero_point_out"),
    ("no workspace", dict(workspace=None), (-3,), "workspace"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_optimize_h16_refuses_hostile_arguments(lib, host_ptr, case):
    _, ptr = host_ptr
    _, over, allowed, word = case
    st = lib.oq_hqq_optimize_h16(*optimize_args(ptr, **over))
    msg = lib.oq_last_error().decode()
    assert st in allowed, (st, msg)
    assert NAME in msg and word in msg, msg


@pytest.mark.parametrize("wtype", [F16, BF16])
def test_optimize_h16_refuses_an_odd_address_and_a_bad_workspace(lib, host_ptr, wtype):
    _, ptr = host_ptr
    st = lib.oq_hqq_optimize_h16(*optimize_args(ptr, wtype=wtype, W=ptr + 1))
    assert st == -1 and "2-byte aligned" in lib.oq_last_error().decode()
    need = lib.oq_hqq_workspace_bytes(128, 64, 64)
    assert 0 < need <= 1 << 19
    st = lib.oq_hqq_optimize_h16(*optimize_args(ptr, wtype=wtype, workspace_bytes=need - 1))
    assert st == -3 and str(need) in lib.oq_last_error().decode()
    st = lib.oq_hqq_optimize_h16(*optimize_args(ptr, wtype=wtype, workspace=ptr + 4))
    assert st == -3 and "8-byte aligned workspace" in lib.oq_last_error().decode()
    for off in (1, 2):                                                           # the blob is written as 4-byte words
        st = lib.oq_hqq_optimize_h16(*optimize_args(ptr, wtype=wtype, layout=NBITS, q_out=ptr + off))
        assert st == -2 and "4-byte aligned output" in lib.oq_last_error().decode()


def test_the_fp32_entry_point_shares_the_checks(lib, host_ptr):
    """One implementation behind both entry points: the same statuses, each message under its own name."""
    _, ptr = host_ptr
    for over, status, word in ((dict(K=0), -1, "K=0"), (dict(K=96, group_size=64), -2, "straddle"), (dict(beta=0.0), -1, "beta"),
                               (dict(workspace_bytes=8), -3, "workspace"), (dict(scale=None), -1, "null scale")):
        args = optimize_args(ptr, **over)
        del args[1]                                                              # no wtype
        st = lib.oq_hqq_optimize_f32(*args)
        msg = lib.oq_last_error().decode()
        assert st == status and "oq_hqq_optimize_f32" in msg and word in msg, (st, msg)
        st = lib.oq_hqq_optimize_h16(*optimize_args(ptr, **over))
        msg16 = lib.oq_last_error().decode()
        assert st == status and msg16 == msg.replace("oq_hqq_optimize_f32", NAME), (st, msg16)
