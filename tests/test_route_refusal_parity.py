"""The tile and the decode entry point of a pair -- oq_matmul_nbits / oq_matmul_nbits_decode, oq_qlinear_matmul /
oq_qlinear_matmul_decode -- make the checks they share through one text (csrc/nbits_common.hpp, csrc/qlinear_epilogue.hpp): for a
hostile call both routes can be given, the two return the same status and, behind the function's name, the same message.  The
workspace cases compare the message with the byte count each route needs masked: the layouts are the routes' own.  Checks that
are worded per route (the group-size unit, the rows of the decode route, the element alignment of the MatMulNBits operands, which
names zero_points on the decode route alone) are held by the four *_abi.py files, not here.

Every library call below is one the checks must REFUSE before any device work, so this file is safe on a box with a GPU too:
the pointers are host memory standing in for device memory and nothing may be launched on them."""
import ctypes as C
import re

import pytest

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
HUGE = (1 << 62) + 12345
F32, F16, ZP_U8 = 0, 1, 3
U8, I8, KN, NK, OUT_I32, OUT_U8 = 0, 1, 0, 1, 0, 2


@pytest.fixture(scope="module")
def lib():
    from onnx_quantize_amd import _build
    from onnx_quantize_amd.hip import _lib
    _build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def host_ptr():
    buf = (C.c_char * (1 << 18))()
    base = C.addressof(buf)
    yield buf, base + (-base % 256)


def nbits_args(ptr, decode, **over):
    # fp16 A, K = 8192: eight slices of K on both routes, 8 * 8 * 16 * 4 = 4096 bytes of slabs each
    a = dict(A=ptr, atype=F16, M=8, K=8192, lda=8192, B=ptr, bits=4, N=16, group_size=32, scales=ptr, scales_type=F32, zero_points=None,
             zero_points_type=ZP_U8, bias=None, flags=0, Y=ptr, ldy=16, workspace=ptr, workspace_bytes=1 << 17, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    if not decode:
        del a["zero_points_type"]
    return list(a.values())


def qlinear_args(ptr, decode, **over):
    a = dict(A=ptr, a_type=U8, M=8, K=2048, lda=2048, a_scale=ptr, a_zero_point=None, B=ptr, b_type=I8, b_layout=NK, N=16, ldb=2048, b_scale=ptr,
             b_zero_point=None, b_per_column=0, C=None, y_scale=ptr, y_zero_point=None, flags=0, out=OUT_U8, Y=ptr, ldy=16, workspace=ptr,
             workspace_bytes=1 << 17, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


EXTENTS = [
    ("M=0", dict(M=0), INVALID), ("M=-1", dict(M=-1), INVALID), ("M=2^62", dict(M=HUGE), INVALID),
    ("K=0", dict(K=0), INVALID), ("K=-1", dict(K=-1), INVALID), ("N=0", dict(N=0), INVALID), ("N=-1", dict(N=-1), INVALID),
    ("N=2^62", dict(N=HUGE, ldy=HUGE), INVALID), ("lda<K", dict(lda=2047), INVALID), ("lda=2^62", dict(lda=HUGE), INVALID),
    ("ldy<N", dict(ldy=15), INVALID), ("ldy=2^62", dict(ldy=HUGE), INVALID),
]
WORKSPACES = [
    ("null workspace", dict(workspace=None), WORKSPACE), ("short workspace", dict(workspace_bytes=64), WORKSPACE),
    ("misaligned workspace", dict(workspace="eight"), WORKSPACE),
]
NBITS_CASES = [
    ("null A", dict(A=None), INVALID), ("null B", dict(B=None), INVALID), ("null scales", dict(scales=None), INVALID), ("null Y", dict(Y=None), INVALID),
    ("atype=3", dict(atype=3), INVALID), ("atype=-1", dict(atype=-1), INVALID), ("scales_type=9", dict(scales_type=9), INVALID),
    ("bf16 scales for fp16 A", dict(scales_type=2), INVALID),
    ("unknown flag", dict(flags=8), INVALID), ("g_idx", dict(flags=2), UNSUPPORTED), ("bits=2", dict(bits=2), UNSUPPORTED),
    *EXTENTS, ("K=2^62", dict(K=HUGE, lda=HUGE), INVALID),
    ("N*K>2^40", dict(N=1 << 30, ldy=1 << 30, K=1 << 11, lda=1 << 11, M=1), INVALID),
    ("all huge", dict(M=HUGE, K=HUGE, N=HUGE, lda=HUGE, ldy=HUGE, group_size=HUGE, workspace_bytes=1 << 62), INVALID),
    ("B off by 8", dict(B="eight"), INVALID), *WORKSPACES,
]
QLINEAR_CASES = [
    ("null A", dict(A=None), INVALID), ("null B", dict(B=None), INVALID), ("null Y", dict(Y=None), INVALID),
    ("null a_scale", dict(a_scale=None), INVALID), ("null b_scale", dict(b_scale=None), INVALID), ("null y_scale", dict(y_scale=None), INVALID),
    ("a_type=5", dict(a_type=5), INVALID), ("b_type=-1", dict(b_type=-1), INVALID), ("b_layout=7", dict(b_layout=7), INVALID),
    ("out=9", dict(out=9), INVALID), ("unknown flag", dict(flags=8), INVALID),
    ("per-row A", dict(flags=1), UNSUPPORTED), ("transA", dict(flags=2), UNSUPPORTED), ("alpha", dict(flags=4), UNSUPPORTED),
    ("every flag", dict(flags=7), UNSUPPORTED),
    *EXTENTS, ("K=2^62", dict(K=HUGE, lda=HUGE, ldb=HUGE), INVALID), ("ldb<K", dict(ldb=2047), INVALID),
    ("ldb<N in KN", dict(b_layout=KN, ldb=15), INVALID), ("N*ldb>2^40", dict(N=1 << 30, ldy=1 << 30, K=1 << 11, M=1), INVALID),
    ("misaligned Y", dict(Y="odd", out=OUT_I32), INVALID), ("misaligned C", dict(C="odd"), INVALID),
    ("misaligned a_scale", dict(a_scale="odd"), INVALID), ("misaligned b_scale", dict(b_scale="odd"), INVALID),
    ("misaligned y_scale", dict(y_scale="odd"), INVALID), *WORKSPACES,
]
PAIRS = {"nbits": ("oq_matmul_nbits", "oq_matmul_nbits_decode", nbits_args), "qlinear": ("oq_qlinear_matmul", "oq_qlinear_matmul_decode", qlinear_args)}
CASES = [("nbits", *c) for c in NBITS_CASES] + [("qlinear", *c) for c in QLINEAR_CASES]


def test_both_routes_of_a_pair_need_a_workspace_at_the_shapes_of_this_file(lib):
    """So that a call whose workspace is hostile is refused by both, and for the same reason."""
    assert lib.oq_matmul_nbits_workspace_bytes(8, 8192, 16, 32, F16) == lib.oq_matmul_nbits_decode_workspace_bytes(8, 8192, 16, 32, F16) == 4096
    assert lib.oq_qlinear_matmul_workspace_bytes(8, 2048, 16) > 64 and lib.oq_qlinear_matmul_decode_workspace_bytes(8, 2048, 16, NK) == 1024


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}: {c[1]}" for c in CASES])
def test_the_tile_and_the_decode_route_refuse_a_shared_hostile_call_alike(lib, host_ptr, case):
    buf, ptr = host_ptr
    pair, _, over, expected = case
    tile, decode, args = PAIRS[pair]
    over = {k: (ptr + 1 if v == "odd" else ptr + 8 if v == "eight" else v) for k, v in over.items()}
    before = bytes(buf)
    answers = []
    for fn, is_decode in ((tile, False), (decode, True)):
        st = getattr(lib, fn)(*args(ptr, is_decode, **over))
        msg = lib.oq_last_error().decode()
        assert st == expected, (fn, st, msg)
        assert msg.startswith(fn + ": "), msg
        text = msg[len(fn) + 2:]
        if expected == WORKSPACE:
            text = re.sub(r"of \d+ bytes is needed", "of # bytes is needed", text)
        answers.append(text)
    assert answers[0] == answers[1]
    assert bytes(buf) == before                                   # nothing written on failure
