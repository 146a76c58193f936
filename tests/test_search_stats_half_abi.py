"""The |x| column statistics of the AWQ / SmoothQuant searches on lists of fp16 / bf16 activations in the half-precision
extension of the C ABI (include/oq_hip_half.h, N2s): the two symbols are declared, bound and exported, the extension version
stays 1, the workspace query is pinned inside and outside the bounds, and hostile tables are refused with the stated status.

Every library call below is one the checks must REFUSE before any device work: the pointers are host memory standing in for
device memory and nothing may be launched on them."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "oq_hip_half.h")
NEW = {"oq_abs_stats_many_half_workspace_bytes": 2, "oq_abs_stats_cols_many_h16": 7}
F16, BF16 = 0, 1
HUGE = (1 << 62) + 12345
FIELDS = ("X", "T", "K", "ldx", "abs_sum", "absmax")


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
    assert raw.oq_half_extension_version() == 1 == _lib.OQ_HALF_EXTENSION_VERSION        # an addition only: the pin stays
    assert re.search(r"const void\* X;\s*int64_t T, K, ldx;\s*float\* abs_sum;\s*float\* absmax;\s*}\s*oq_abs_stats_item;", text)


# ------------------------------------------------------------------------------------ tables in host memory
@pytest.fixture(scope="module")
def host():
    """(buffer, 16-byte aligned address in it).  Items point at [base + 4096, ...) for X and [base + 32768, ...) for the outputs;
    the tables themselves are separate arrays, so 'nothing written' covers everything an item points at."""
    buf = (C.c_char * (1 << 16))()
    base = C.addressof(buf)
    yield buf, base + (-base % 16)


def _item(ptr, i=0, **over):
    it = dict(X=ptr + 4096 + 2048 * i, T=64, K=32, ldx=32, abs_sum=ptr + 32768 + 512 * i, absmax=ptr + 32768 + 512 * i + 256)
    assert set(over) <= set(it)
    it.update(over)
    return [it[f] or 0 for f in FIELDS]


def _table(items):
    flat = [v for it in items for v in it]
    return (C.c_int64 * len(flat))(*flat)


def _refused(lib, table, count, buf, allowed, word, xtype=F16, device="table", workspace="ok", workspace_bytes=1 << 20):
    ptr = C.addressof(buf) + (-C.addressof(buf) % 16)
    before = bytes(buf)
    dev = None if device is None or table is None else C.addressof(table) + (4 if device == "odd" else 0)
    ws = None if workspace is None else ptr + 49152
    st = lib.oq_abs_stats_cols_many_h16(C.addressof(table) if table is not None else None, dev, count, xtype, ws, workspace_bytes, None)
    msg = lib.oq_last_error().decode()
    assert st in allowed, (st, msg)
    assert word in msg, msg
    assert bytes(buf) == before                                   # nothing written on failure


ITEM_CASES = [
    # (what is hostile, overrides of item 1 of 3, a word of the message)
    ("null X", dict(X=None), "null"), ("null abs_sum", dict(abs_sum=None), "null"), ("null absmax", dict(absmax=None), "null"),
    ("odd X", dict(X="odd"), "2-byte aligned"), ("odd abs_sum", dict(abs_sum="odd"), "4-byte aligned"),
    ("T=0", dict(T=0), "T=0"), ("T=-1", dict(T=-1), "T=-1"), ("T=2^62", dict(T=HUGE), "T="), ("T=2^31", dict(T=1 << 31), "T="),
    ("K=0", dict(K=0), "K=0"), ("K=-1", dict(K=-1), "K=-1"), ("K=2^62", dict(K=HUGE, ldx=HUGE), "K="),
    ("ldx<K", dict(ldx=31), "ldx=31"), ("ldx=2^62", dict(ldx=HUGE), "ldx="), ("ldx=2^31", dict(ldx=1 << 31), "ldx="),
    ("T*ldx>2^40", dict(T=1 << 30, ldx=1 << 11), "T="), ("all huge", dict(T=HUGE, K=HUGE, ldx=HUGE), "T="),
]


@pytest.mark.parametrize("case", ITEM_CASES, ids=[c[0] for c in ITEM_CASES])
def test_a_hostile_item_is_refused_and_named(lib, host, case):
    buf, ptr = host
    over = {k: (ptr + 4096 + 1 if v == "odd" else v) for k, v in case[1].items()}
    table = _table([_item(ptr, 0), _item(ptr, 1, **over), _item(ptr, 2)])
    before = bytes(table)
    _refused(lib, table, 3, buf, (-1,), case[2])
    assert "item 1" in lib.oq_last_error().decode()
    assert bytes(table) == before
    if "X" not in case[1] and "abs_sum" not in case[1] and "absmax" not in case[1]:      # the query looks at extents only
        assert lib.oq_abs_stats_many_half_workspace_bytes(C.addressof(table), 3) == 0


def test_hostile_call_arguments_are_refused(lib, host):
    buf, ptr = host
    table = _table([_item(ptr, 0), _item(ptr, 1)])
    _refused(lib, table, 2, buf, (-1,), "xtype", xtype=2)
    _refused(lib, table, 2, buf, (-1,), "xtype", xtype=-1)
    _refused(lib, None, 2, buf, (-1,), "null items_host")
    for count in (0, -1, 65536, HUGE, -HUGE):
        _refused(lib, table, count, buf, (-1,), "count=")
    _refused(lib, table, 2, buf, (-1,), "items_device", device=None)           # NULL only when count == 1
    _refused(lib, table, 2, buf, (-1,), "8-byte aligned", device="odd")
    need = lib.oq_abs_stats_many_half_workspace_bytes(C.addressof(table), 2)
    assert need == 2 * 64 * 32 * 8 + 256
    _refused(lib, table, 2, buf, (-3,), "workspace", workspace=None)
    _refused(lib, table, 2, buf, (-3,), str(need), workspace_bytes=need - 1)
    _refused(lib, table, 2, buf, (-3,), str(need), workspace_bytes=0)
    # a NULL device table with count == 1 gets past that check: the next hostile thing is what is reported
    _refused(lib, table, 1, buf, (-3,), "workspace", device=None, workspace=None)
    # everything hostile at once: the first check answers
    bad = _table([_item(ptr, 0, T=HUGE, K=HUGE, ldx=HUGE)])
    _refused(lib, bad, HUGE, buf, (-1,), "xtype", xtype=7, workspace=None, workspace_bytes=0)


# ------------------------------------------------------------------------------------ workspace query
def test_workspace_query_inside_the_bounds(lib, host):
    _, ptr = host
    q = lib.oq_abs_stats_many_half_workspace_bytes
    # count slots of max over the items of min(T, 64) * K floats, twice (sums, maxima), + 256
    one = _table([_item(ptr, 0, T=1, K=1, ldx=1)])
    assert q(C.addressof(one), 1) == 8 + 256
    t = _table([_item(ptr, 0, T=3, K=7, ldx=9)])
    assert q(C.addressof(t), 1) == 3 * 7 * 8 + 256
    t = _table([_item(ptr, 0, T=5120, K=640, ldx=640), _item(ptr, 1, T=5, K=2048, ldx=2048), _item(ptr, 2, T=5120, K=1024, ldx=4096)])
    assert q(C.addressof(t), 3) == 3 * 64 * 1024 * 8 + 256
    assert q(C.addressof(t), 2) == 2 * 64 * 640 * 8 + 256
    big = _table([_item(ptr, 0, T=(1 << 31) - 1, K=1, ldx=512), _item(ptr, 1, T=512, K=(1 << 31) - 1, ldx=(1 << 31) - 1)])
    assert q(C.addressof(big), 2) == 2 * 64 * ((1 << 31) - 1) * 8 + 256
    pointers_do_not_matter = _table([_item(ptr, 0, X=None, abs_sum=None, absmax=None)])
    assert q(C.addressof(pointers_do_not_matter), 1) == 64 * 32 * 8 + 256


@pytest.mark.parametrize("count", [0, -1, 65536, HUGE, -HUGE])
def test_workspace_query_returns_zero_for_a_count_outside_the_bounds(lib, host, count):
    _, ptr = host
    table = _table([_item(ptr, 0)])
    assert lib.oq_abs_stats_many_half_workspace_bytes(C.addressof(table), count) == 0


def test_workspace_query_returns_zero_for_a_null_table(lib):
    assert lib.oq_abs_stats_many_half_workspace_bytes(None, 1) == 0
