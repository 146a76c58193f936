"""Calibration statistics of fp16 / bf16 activations in the half-precision extension of the C ABI (include/oq_hip_half.h):
the six symbols are declared, bound and exported, their argument checks answer without a GPU, the workspace queries are
pinned inside and outside the bounds, and no kernel of csrc/reduce_half.hip spills.

Every library call below is one the checks must REFUSE before any device work: the pointers are host memory standing in for
device memory and nothing may be launched on them."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from kernel_report import HALF_ELEMS, element_types, needs_hipcc, report

HEADER = os.path.join(ROOT, "include", "oq_hip_half.h")
NEW = {"oq_minmax_half_workspace_bytes": 1, "oq_minmax_collect_h16": 8, "oq_minmax_many_half_workspace_bytes": 1,
       "oq_minmax_collect_many_h16": 7, "oq_absmax_half_workspace_bytes": 3, "oq_absmax_h16": 10}


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
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(oq_[a-z0-9_]+)\s*\(", text))
    raw = C.CDLL(lib_path)
    for name, nargs in NEW.items():
        assert name in declared, f"{name} is not declared in include/oq_hip_half.h"
        assert name in _lib.HALF_PROTOTYPES, f"{name} is not in _lib.HALF_PROTOTYPES"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert len(_lib.HALF_PROTOTYPES[name][1]) == nargs, name
    assert declared == set(_lib.HALF_PROTOTYPES)                                           # header and binding stay one set
    assert raw.oq_half_extension_version() == 1 == _lib.OQ_HALF_EXTENSION_VERSION        # additions only: the pin stays


# ------------------------------------------------------------------------------------ hostile arguments
F16, BF16 = 0, 1
HUGE = (1 << 62) + 12345
MINMAX_WS = 2048 * 2 * 4                        # one (min, max) pair of floats for each of at most 2048 blocks


@pytest.fixture(scope="module")
def host_ptr():
    buf = (C.c_char * (1 << 16))()
    base = C.addressof(buf)
    yield buf, base + (-base % 16)


def _refused(lib, fn, args, buf, allowed, word):
    before = bytes(buf)
    st = fn(*args)
    msg = lib.oq_last_error().decode()
    assert st in allowed, (st, msg)
    assert word in msg, msg
    assert bytes(buf) == before                                   # nothing written on failure


def _args(defaults, ptr, over):
    assert set(over) <= set(defaults)
    a = {**defaults, **{k: (ptr + 1 if v == "odd" else v) for k, v in over.items()}}
    return list(a.values())


COLLECT_CASES = [
    # (what is hostile, overrides, statuses allowed, a word of the message)
    ("null x", dict(x=None), (-1,), "null"), ("null state", dict(state=None), (-1,), "null"),
    ("odd x", dict(x="odd"), (-1,), "2-byte aligned"),
    ("xtype=2", dict(xtype=2), (-1,), "xtype"), ("xtype=-1", dict(xtype=-1), (-1,), "xtype"),
    ("count=0", dict(count=0), (-1,), "count=0"), ("count=-1", dict(count=-1), (-1,), "count=-1"),
    ("count=2^40+1", dict(count=(1 << 40) + 1), (-1,), "count="), ("count=2^62", dict(count=HUGE), (-1,), "count="),
    ("momentum=1", dict(momentum=1.0), (-1,), "Momentum"), ("momentum=-0.1", dict(momentum=-0.1), (-1,), "Momentum"),
    ("momentum=nan", dict(momentum=float("nan")), (-1,), "Momentum"),
    ("null workspace", dict(workspace=None), (-3,), "workspace"),
    ("short workspace", dict(workspace_bytes=MINMAX_WS - 1), (-3,), str(MINMAX_WS)),
    ("all hostile", dict(count=HUGE, momentum=7.0, workspace_bytes=0), (-1,), "count="),
]


@pytest.mark.parametrize("case", COLLECT_CASES, ids=[c[0] for c in COLLECT_CASES])
def test_collect_h16_refuses_hostile_arguments(lib, host_ptr, case):
    buf, ptr = host_ptr
    defaults = dict(x=ptr, xtype=F16, count=4096, state=ptr + 32768, momentum=0.0, workspace=ptr + 40000, workspace_bytes=MINMAX_WS, stream=None)
    _refused(lib, lib.oq_minmax_collect_h16, _args(defaults, ptr, case[1]), buf, case[2], case[3])


MANY_CASES = [
    ("null desc", dict(desc=None), (-1,), "null"), ("odd desc", dict(desc="odd"), (-1,), "aligned"),
    ("xtype=2", dict(xtype=2), (-1,), "xtype"), ("xtype=-1", dict(xtype=-1), (-1,), "xtype"),
    ("n=0", dict(n=0), (-1,), "n=0"), ("n=-1", dict(n=-1), (-1,), "n=-1"), ("n=65536", dict(n=65536), (-1,), "n=65536"),
    ("n=2^62", dict(n=HUGE), (-1,), "n="),
    ("momentum=1", dict(momentum=1.0), (-1,), "Momentum"), ("momentum=-0.1", dict(momentum=-0.1), (-1,), "Momentum"),
    ("null workspace", dict(workspace=None), (-3,), "workspace"),
    ("short workspace", dict(workspace_bytes=3 * 64 * 8 + 255), (-3,), str(3 * 64 * 8 + 256)),
]


@pytest.mark.parametrize("case", MANY_CASES, ids=[c[0] for c in MANY_CASES])
def test_collect_many_h16_refuses_hostile_arguments(lib, host_ptr, case):
    buf, ptr = host_ptr
    defaults = dict(desc=ptr, n=3, xtype=BF16, momentum=0.0, workspace=ptr + 4096, workspace_bytes=1 << 15, stream=None)
    _refused(lib, lib.oq_minmax_collect_many_h16, _args(defaults, ptr, case[1]), buf, case[2], case[3])


ABSMAX_CASES = [
    ("null x", dict(x=None), (-1,), "null"), ("null out", dict(out=None), (-1,), "null"),
    ("odd x", dict(x="odd"), (-1,), "2-byte aligned"),
    ("xtype=2", dict(xtype=2), (-1,), "xtype"), ("xtype=-1", dict(xtype=-1), (-1,), "xtype"),
    ("R=0", dict(R=0), (-1,), "R=0"), ("R=-1", dict(R=-1), (-1,), "R=-1"), ("R=2^62", dict(R=HUGE), (-1,), "R="),
    ("C=0", dict(C=0), (-1,), "C=0"), ("C=-1", dict(C=-1), (-1,), "C=-1"), ("C=2^62", dict(C=HUGE, ldx=HUGE), (-1,), "C="),
    ("ldx<C", dict(ldx=31), (-1,), "ldx=31"), ("ldx=2^62", dict(ldx=HUGE), (-1,), "ldx="),
    ("R*ldx>2^40", dict(R=1 << 30, ldx=1 << 11), (-1,), "R="),
    ("all huge", dict(R=HUGE, C=HUGE, ldx=HUGE, workspace_bytes=1 << 62), (-1,), "R="),
    ("rows, R=2^62", dict(R=HUGE, transposed=1), (-1,), "R="),
    ("null workspace", dict(workspace=None), (-3,), "workspace"),
    ("short workspace", dict(R=300, workspace_bytes=3 * 32 * 4 - 1), (-3,), str(3 * 32 * 4)),
]


@pytest.mark.parametrize("case", ABSMAX_CASES, ids=[c[0] for c in ABSMAX_CASES])
def test_absmax_h16_refuses_hostile_arguments(lib, host_ptr, case):
    buf, ptr = host_ptr
    defaults = dict(x=ptr, xtype=F16, R=64, C=32, ldx=32, transposed=0, out=ptr + 32768, workspace=ptr + 40000, workspace_bytes=1 << 14, stream=None)
    _refused(lib, lib.oq_absmax_h16, _args(defaults, ptr, case[1]), buf, case[2], case[3])


# ------------------------------------------------------------------------------------ workspace queries
def test_workspace_queries_inside_the_bounds(lib):
    assert lib.oq_minmax_half_workspace_bytes(1) == MINMAX_WS == lib.oq_minmax_half_workspace_bytes(1 << 40)
    # n tensors x slices (4096 / n, clamped to 4 .. 64) x (min, max) floats, + 256
    assert lib.oq_minmax_many_half_workspace_bytes(1) == 64 * 8 + 256
    assert lib.oq_minmax_many_half_workspace_bytes(72) == 72 * 56 * 8 + 256
    assert lib.oq_minmax_many_half_workspace_bytes(65535) == 65535 * 4 * 8 + 256
    # columns: one float per column and chunk of 128 rows, + 256; rows: nothing is kept
    assert lib.oq_absmax_half_workspace_bytes(64, 32, 0) == 32 * 4 + 256
    assert lib.oq_absmax_half_workspace_bytes(129, 33, 0) == 2 * 33 * 4 + 256
    assert lib.oq_absmax_half_workspace_bytes(129, 33, 1) == 256


@pytest.mark.parametrize("count", [0, -1, (1 << 40) + 1, HUGE, -HUGE])
def test_minmax_workspace_query_returns_zero_outside_the_bounds(lib, count):
    assert lib.oq_minmax_half_workspace_bytes(count) == 0


@pytest.mark.parametrize("n", [0, -1, 65536, HUGE, -HUGE])
def test_many_workspace_query_returns_zero_outside_the_bounds(lib, n):
    assert lib.oq_minmax_many_half_workspace_bytes(n) == 0


@pytest.mark.parametrize("shape", [(0, 32), (-1, 32), (HUGE, 32), (64, 0), (64, -1), (64, HUGE), (1 << 31, 4), (1 << 30, 1 << 11), (HUGE, HUGE)])
@pytest.mark.parametrize("transposed", [0, 1])
def test_absmax_workspace_query_returns_zero_outside_the_bounds(lib, shape, transposed):
    assert lib.oq_absmax_half_workspace_bytes(*shape, transposed) == 0


# ------------------------------------------------------------------------------------ kernel resources
@needs_hipcc
def test_reduce_half_kernels_do_not_spill():
    """HBM-bound streams: eight 16-byte loads per lane are 32 registers; scratch traffic would compete with the stream itself."""
    seen = report("reduce_half.hip").kernels
    for key in ("minmax_half_partial", "absmax_half_cols_partial", "absmax_half_rows"):
        assert element_types(seen, key) == HALF_ELEMS, (key, list(seen))               # fp16 and bf16 instantiations
    for key in ("minmax_half_update", "absmax_half_cols_finalize"):
        assert sum(key in name for name in seen) == 1, (key, list(seen))
    assert len(seen) == 8, list(seen)
    for name, k in seen.items():
        assert k.scratch == 0 and k.sgpr_spill == 0 and k.vgpr_spill == 0, (name, k)
        assert k.occupancy >= 4, (name, k)                  # 512-thread blocks, two per CU at the least: <= 128 registers
