"""oq_rtn_quantize_ptrs_h16 (include/oq_hip_half.h): RTN on a LIST of fp16 / bf16 matrices, a device table of pointers per call.
Its argument checks answer without a GPU: they read the HOST copy of the table, before any arithmetic on an extent and before any
HIP call.

Every call of the sweep below is one the checks must REFUSE, so this file is safe on a box with a GPU too: the pointers are host
memory standing in for device memory and nothing may be launched on them."""
import ctypes as C
import inspect

import pytest

F16, UINT4, UINT8, KN, NBITS, PACKED4 = 0, 1, 3, 0, 1, 2
INVALID, UNSUPPORTED = -1, -2
EXTENT = (1 << 31) - 1          # oq_common.hpp: kMaxExtent; rows * ldw <= 2^40 (kMaxElements)
HUGE = (1 << 62) + 12345


@pytest.fixture(scope="module")
def lib():
    from onnx_quantize_amd import _build
    from onnx_quantize_amd.hip import _lib
    _build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def host():
    buf = (C.c_char * (1 << 16))()
    base = C.addressof(buf)
    yield buf, base + (-base % 16)


def table_of(ptr, count, edits=None):
    """`count` entries {W, q_out, scale_out, zp_out}, all at the aligned host address; edits: {(entry, field): value}."""
    t = (C.c_int64 * (4 * max(count, 1)))(*([ptr] * (4 * max(count, 1))))
    for (entry, field), value in (edits or {}).items():
        t[4 * entry + field] = value
    return t


def call(lib, ptr, table="host", device="host", edits=None, **over):
    a = dict(count=3, wtype=F16, K=256, N=64, ldw=64, qtype=UINT4, group_size=128, symmetric=0, reduce_range=0, clip_ratio=1.0, layout=KN)
    assert set(over) <= set(a)
    a.update(over)
    t = table_of(ptr, min(max(a["count"], 1), 8), edits)
    th = C.addressof(t) if table == "host" else None
    td = C.addressof(t) if device == "host" else None
    st = lib.oq_rtn_quantize_ptrs_h16(th, td, a["count"], a["wtype"], a["K"], a["N"], a["ldw"], a["qtype"], a["group_size"], a["symmetric"],
                                      a["reduce_range"], a["clip_ratio"], a["layout"], None)
    return st, lib.oq_last_error().decode()


CASES = [
    # (what is hostile, keyword arguments of `call`, statuses allowed, a word of the message)
    ("null table_host", dict(table=None), (INVALID,), "table_host"),
    ("null table_device, count 2", dict(device=None, count=2), (INVALID,), "table_device"),
    ("count 0", dict(count=0), (INVALID,), "count 0"), ("count -1", dict(count=-1), (INVALID,), "count -1"),
    ("count 65536", dict(count=65536), (INVALID,), "count 65536"),
    ("wtype 2", dict(wtype=2), (INVALID,), "wtype"), ("wtype -1", dict(wtype=-1), (INVALID,), "wtype"),
    ("K=0", dict(K=0), (INVALID,), "K=0"), ("K=-1", dict(K=-1), (INVALID,), "K=-1"),
    ("K beyond", dict(K=EXTENT + 1), (UNSUPPORTED,), "too large"), ("K=2^62", dict(K=HUGE), (UNSUPPORTED,), "too large"),
    ("K at the bound, K * ldw beyond", dict(K=EXTENT, N=1024, ldw=1024, group_size=1), (UNSUPPORTED,), "too large"),
    ("N=0", dict(N=0, ldw=0), (INVALID,), "N=0"), ("N beyond", dict(N=EXTENT + 1, ldw=EXTENT + 1), (UNSUPPORTED,), "too large"),
    ("ldw<N", dict(ldw=63), (INVALID,), "ldw=63"), ("ldw beyond", dict(ldw=EXTENT + 1), (UNSUPPORTED,), "too large"),
    ("ldw at the bound, K * ldw beyond", dict(K=1024, ldw=EXTENT), (UNSUPPORTED,), "too large"),
    ("all huge", dict(K=HUGE, N=HUGE, ldw=HUGE, group_size=HUGE), (UNSUPPORTED,), "too large"),
    ("straddling groups", dict(group_size=96), (UNSUPPORTED,), "group_size 96"),
    ("g=512", dict(K=1024, group_size=512), (UNSUPPORTED,), "group_size 512"),
    ("g=-1 of K=512", dict(K=512, group_size=-1), (UNSUPPORTED,), "group_size 512"),
    ("group_size=0", dict(group_size=0), (INVALID,), "group_size"),
    ("clip 0", dict(clip_ratio=0.0), (INVALID,), "clip_ratio"), ("clip 1.5", dict(clip_ratio=1.5), (INVALID,), "clip_ratio"),
    ("clip nan", dict(clip_ratio=float("nan")), (INVALID,), "clip_ratio"),
    ("layout 9", dict(layout=9), (INVALID,), "layout"), ("qtype 99", dict(qtype=99), (INVALID,), "quantization type"),
    ("nbits, g=24", dict(K=96, group_size=24, layout=NBITS), (UNSUPPORTED,), "group_size % 16"),
    ("nbits, q_out of entry 1 off by 8", dict(layout=NBITS, edits={(1, 1): 8}), (UNSUPPORTED,), "entry 1"),
    ("packed4, 8-bit type", dict(layout=PACKED4, qtype=UINT8), (UNSUPPORTED,), "4-bit"),
    ("packed4, odd N", dict(layout=PACKED4, N=63, ldw=64), (UNSUPPORTED,), "N=63"),
    ("packed4, g=48", dict(layout=PACKED4, K=96, group_size=48), (UNSUPPORTED,), "wave kernel"),
    ("W of entry 2 at an odd address", dict(edits={(2, 0): 1}), (INVALID,), "entry 2"),
    ("scale_out of entry 1 off by 2", dict(edits={(1, 2): 2}), (INVALID,), "entry 1"),
    ("null q_out in entry 2", dict(edits={(2, 1): None}), (INVALID,), "entry 2"),
    ("null zp_out in entry 0", dict(edits={(0, 3): None}), (INVALID,), "entry 0"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_ptrs_h16_refuses_hostile_arguments(lib, host, case):
    _, ptr = host
    _, kw, allowed, word = case
    kw = dict(kw)
    if "edits" in kw:      # offsets are relative to the aligned host address; None is a null pointer
        kw["edits"] = {key: 0 if off is None else ptr + off for key, off in kw["edits"].items()}
    st, msg = call(lib, ptr, **kw)
    assert st in allowed, (st, msg)
    assert word in msg, msg


def test_the_list_route_exists_and_the_fp32_only_entry_points_name_it():
    import torch
    from onnx_quantize_amd.hip import _lib, ops
    assert "oq_rtn_quantize_ptrs_h16" in _lib.HALF_PROTOTYPES
    sig = inspect.signature(ops.rtn_quantize_model)
    assert list(sig.parameters) == ["ws", "qtype", "group_size", "symmetric", "reduce_range", "clip_ratio", "layout"]
    assert sig.parameters["layout"].default == "kn" and sig.parameters["clip_ratio"].default == 1.0
    assert ops.rtn_quantize_model([], "uint4", 128) == []
    with pytest.raises(TypeError, match="rtn_quantize_model") as e:
        ops._refuse_half(torch.zeros((2, 2), dtype=torch.bfloat16), "rtn_quantize_many")
    assert "rtn_quantize_many" in str(e.value) and "rtn_quantize " in str(e.value)
