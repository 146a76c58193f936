"""The grouped GPTQ Hessian of fp16 / bf16 activations (oq_hessian_accumulate_many_h16, include/oq_hip_half.h): declared, bound
and exported, its argument checks answer on the host, and its workspace query follows the formula the header states.

Every library call below is one the checks must REFUSE before any device work: the item tables, the X / H pointers inside them
and the workspace are host memory standing in for device memory, and nothing may be launched on them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "oq_hip_half.h")
NEW = {"oq_hessian_many_half_workspace_bytes": 2, "oq_hessian_accumulate_many_h16": 7}
F16, BF16 = 0, 1
HUGE = (1 << 62) + 12345


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
        assert len(_lib.HALF_PROTOTYPES[name][1]) == nargs, name
        assert hasattr(raw, name), f"{name} is not exported by the library"
    assert raw.oq_half_extension_version() == 1 == _lib.OQ_HALF_EXTENSION_VERSION        # an addition only: the pin stays


# ------------------------------------------------------------------------------------ hostile arguments
@pytest.fixture(scope="module")
def host_ptr():
    buf = (C.c_char * (1 << 16))()
    base = C.addressof(buf)
    yield buf, base + (-base % 16)


def table(ptr, middle=None, count=3):
    """`count` well-formed items (X and H inside the guarded buffer); `middle` overrides fields of item 1."""
    items = [dict(X=ptr, H=ptr + 4096, T=64, K=32, ldx=32, n_seen=0, n_add=4, reserved=0) for _ in range(count)]
    if middle:
        assert set(middle) <= set(items[1])
        items[1].update(middle)
    return np.asarray([list(i.values()) for i in items], dtype=np.int64)


def call(lib, ptr, items, **over):
    a = dict(items_host=C.c_void_p(items.ctypes.data), items_device=C.c_void_p(items.ctypes.data), count=len(items), xtype=F16,
             workspace=ptr + 8192, workspace_bytes=1 << 15, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return lib.oq_hessian_accumulate_many_h16(*a.values())


CALL_CASES = [
    # (what is hostile, overrides of the call, overrides of the middle item, statuses allowed, a word of the message)
    ("count=0", dict(count=0), None, (-1,), "count=0"), ("count=-1", dict(count=-1), None, (-1,), "count=-1"),
    ("count=65536", dict(count=65536), None, (-1,), "count=65536"),
    ("null host table", dict(items_host=None), None, (-1,), "null"), ("null device table", dict(items_device=None), None, (-1,), "null"),
    ("null X", None, dict(X=0), (-1,), "item 1: null"), ("null H", None, dict(H=0), (-1,), "item 1: null"),
    ("odd X", None, dict(X="odd"), (-1,), "item 1: X must be 2-byte aligned"),
    ("T=0", None, dict(T=0), (-1,), "item 1: bad shape T=0"), ("T=2^62", None, dict(T=HUGE), (-1, -2), "item 1"),
    ("K=0", None, dict(K=0), (-1,), "K=0"),
    ("K>2^17", None, dict(K=(1 << 17) + 1, ldx=(1 << 17) + 1), (-2,), "item 1: operand too large"),
    ("ldx<K", None, dict(ldx=31), (-1,), "ldx=31"),
    ("n_add=0", None, dict(n_add=0), (-1,), "item 1: bad sample counts"), ("n_seen=-1", None, dict(n_seen=-1), (-1,), "sample counts"),
    ("T*ldx>2^40", None, dict(T=1 << 30, K=32, ldx=1 << 11), (-2,), "item 1: operand too large"),
    ("xtype=7", dict(xtype=7), None, (-1,), "xtype 7"), ("xtype=-1", dict(xtype=-1), None, (-1,), "xtype"),
    ("null workspace", dict(workspace=None), None, (-3,), "workspace"), ("short workspace", dict(workspace_bytes=64), None, (-3,), "workspace"),
]


@pytest.mark.parametrize("case", CALL_CASES, ids=[c[0] for c in CALL_CASES])
def test_accumulate_many_h16_refuses_hostile_arguments(lib, host_ptr, case):
    buf, ptr = host_ptr
    _, over, middle, allowed, word = case
    if middle:
        middle = {k: (ptr + 1 if v == "odd" else v) for k, v in middle.items()}
    items = table(ptr, middle)
    kept = items.copy()
    before = bytes(buf)
    st = call(lib, ptr, items, **(over or {}))
    msg = lib.oq_last_error().decode()
    assert st in allowed, (st, msg)
    assert word in msg, msg
    assert bytes(buf) == before and np.array_equal(items, kept)          # nothing written on failure


def test_a_well_formed_table_passes_the_item_checks_and_stops_at_the_workspace(lib, host_ptr):
    """The table of the hostile cases is refused for what each case changes, not for something else: unchanged, it gets as far as
    the workspace check, whose message states the queried size."""
    buf, ptr = host_ptr
    items = table(ptr)
    need = lib.oq_hessian_many_half_workspace_bytes(C.c_void_p(items.ctypes.data), 3)
    assert need > 64
    assert call(lib, ptr, items, workspace_bytes=need - 1) == -3
    assert f"{need} bytes needed, {need - 1} given" in lib.oq_last_error().decode()


# ------------------------------------------------------------------------------------ workspace query
def query(lib, items, count=None):
    return lib.oq_hessian_many_half_workspace_bytes(C.c_void_p(items.ctypes.data) if items is not None else None, len(items) if count is None else count)


QUERY_CASES = [("count=0", None, dict(count=0)), ("count=-1", None, dict(count=-1)), ("count=65536", None, dict(count=65536)),
               ("T=0", dict(T=0), {}), ("T=-1", dict(T=-1), {}), ("T=2^62", dict(T=HUGE), {}), ("K=0", dict(K=0), {}), ("K=2^62", dict(K=HUGE), {}),
               ("K>2^17", dict(K=(1 << 17) + 1), {}), ("T*K>2^40", dict(T=1 << 24, K=1 << 17), {})]


@pytest.mark.parametrize("case", QUERY_CASES, ids=[c[0] for c in QUERY_CASES])
def test_workspace_query_returns_zero_outside_the_bounds(lib, host_ptr, case):
    _, middle, kw = case
    assert query(lib, table(host_ptr[1], middle), **kw) == 0


def test_workspace_query_of_a_null_table_is_zero(lib):
    assert lib.oq_hessian_many_half_workspace_bytes(None, 3) == 0


def test_workspace_query_inside_the_bounds(lib, host_ptr):
    """The header's formula: count * 128 of table rounded up to 256, T padded to 32 x K padded to 256 x 2 bytes per item, + 512."""
    ptr = host_ptr[1]
    assert query(lib, table(ptr)) == 512 + 3 * (64 * 256 * 2) + 512                                   # 3 * 128 = 384 -> 512
    items = table(ptr, dict(T=33, K=257, ldx=259), count=2)
    assert query(lib, items) == 256 + (64 * 256 * 2 + 64 * 512 * 2) + 512
    assert query(lib, items, count=1) == 256 + 64 * 256 * 2 + 512                                      # the first item alone
