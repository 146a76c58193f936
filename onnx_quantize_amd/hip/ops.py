"""Device-level operators: torch tensors in HBM in, torch tensors in HBM out.

torch is plumbing here (device memory, streams); every computation is a call through the
C ABI of liboq_hip.so on the current torch stream.  No function in this module has a CPU
implementation: a missing library or a non-CUDA tensor is an error.
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np
import torch

from . import _lib as L

_CONTAINER = {"int4": torch.int8, "uint4": torch.uint8, "int8": torch.int8, "uint8": torch.uint8,
              "int32": torch.int32, "uint32": torch.uint32}
BITS = {"int4": 4, "uint4": 4, "int8": 8, "uint8": 8, "int32": 32, "uint32": 32}


def container_dtype(qtype: str) -> torch.dtype:
    return _CONTAINER[qtype]


_LAYOUTS = {"kn": L.OQ_LAYOUT_KN, "nbits": L.OQ_LAYOUT_NBITS, "kn_packed4": L.OQ_LAYOUT_KN_PACKED4}


def _layout_code(layout: str) -> int:
    if layout not in _LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(_LAYOUTS)}, got {layout!r}")
    return _LAYOUTS[layout]


def _q_buffer(layout: str, lead: tuple, k: int, n: int, g: int, qtype: str, device):
    """The integer output of one matrix (or a stack: ``lead``) in the requested layout: [K, N] one value per byte, the
    MatMulNBits blob [N, K/g, g*bits/8], or [K, N/2] packed nibbles (core/_pack.py:8-22 order)."""
    _layout_code(layout)
    if layout == "kn":
        return torch.empty((*lead, k, n), dtype=container_dtype(qtype), device=device)
    if layout == "kn_packed4":
        if BITS[qtype] != 4 or n % 2:
            raise ValueError("layout 'kn_packed4' takes a 4-bit type and an even number of columns")
        return torch.empty((*lead, k, n // 2), dtype=torch.uint8, device=device)
    return torch.empty((*lead, n, k // g, g * BITS[qtype] // 8), dtype=torch.uint8, device=device)


def _ptr(t: torch.Tensor | None) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _item_table(rows, device):
    """The per-item integer rows of a list entry point as the library takes them: (the contiguous int64 host array, its
    pointer, its device copy -- one blocking copy; None for ``device`` None: an entry point that reads a list of one from the host)."""
    host = np.asarray(rows, dtype=np.int64)
    return host, C.c_void_p(host.ctypes.data), None if device is None else torch.from_numpy(host).to(device)


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw_stream(device_index: int) -> int:
    """The handle of the current stream of a device, without building a `torch.cuda.Stream` around it where torch offers that."""
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    return raw(device_index) if raw is not None else torch.cuda.current_stream(device_index).cuda_stream


def _require_device(t: torch.Tensor, name: str, dtype=None) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name} must be a torch tensor in GPU memory (the HIP path has no CPU fallback)")
    if t.device.index != torch.cuda.current_device():
        # the library launches on the CURRENT device's current stream and never switches devices itself
        raise RuntimeError(f"{name} lives on {t.device} but the current device is cuda:{torch.cuda.current_device()}: "
                           f"call inside `with torch.cuda.device({t.device.index}):`")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")


_ARENA_MIN_BYTES = 32 << 20
_ARENA_MAX_STREAMS = 4
_ARENA: dict = {}       # the scratch tensors of `_workspace`
_RTN_STATE: dict = {}    # the zero-filled state of the one-read channel / tensor RTN kernels
_MINMAX_WS: dict = {}    # the workspace reused by every `minmax_collect` on a stream (plain dicts: that call reads its own with one `get`)


def _stream_buffer(cache: dict, device, nbytes: int, alloc) -> torch.Tensor:
    """What the three caches above have in common.  ``cache``: (device index, stream handle) -> ONE buffer of that stream, grow-only,
    most recently used last, at most `_ARENA_MAX_STREAMS` entries; calls on a stream run in order, so the next call may
    overwrite what the previous one left.  Returns the buffer of ``device``'s current stream, of at least ``nbytes``: a missing
    or smaller one is replaced by ``alloc(nbytes, device)``.  "Used" means a call of this function: `minmax_collect` reads
    `_MINMAX_WS` with a plain `get` on a hit, so that cache orders its streams by first use and a busy stream can lose its (small)
    workspace to four newer ones; it then takes a new one here."""
    dev = torch.device(device)
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (index, torch.cuda.current_stream(index).cuda_stream)
    buf = cache.pop(key, None)
    if buf is None or buf.numel() < nbytes:
        del buf
        buf = alloc(nbytes, torch.device("cuda", index))
    cache[key] = buf                                   # (re-)inserted last: dicts keep insertion order
    while len(cache) > _ARENA_MAX_STREAMS:             # a caller cycling through many streams must not pin one buffer per stream:
        cache.pop(next(iter(cache)))                   # the least recently used one goes back to torch's allocator (stream-ordered)
    return buf


def _workspace(nbytes: int, device, keep: bool = False) -> torch.Tensor | None:
    """Scratch memory for ONE library call on the current stream.  Nothing a call returns lives in it.

    Small requests come from torch's allocator.  Requests of 32 MiB and more (the factor chain of a stack of eight
    11008 x 11008 Hessians asks for 15.5 GB) are served from one grow-only buffer per (device, stream): calls on a stream run
    in order, so the next call may overwrite what the previous one left; at most four streams keep one (least recently used
    out).  Why not `torch.empty` every time: when the
    caching allocator has split its one block of that size for a smaller request in between, the next call maps a new one,
    and `hipMalloc` of 15.5 GB takes 0.36 s on the MI355X host (measured, scripts/lab_alloc_trace.py) -- with the kernels of
    the call waiting behind it.  `release_workspaces()` hands the buffers back.  ``keep``: a small request is served from that
    buffer as well (HQQ: the trajectory of every round, about a byte per weight next to an output of one byte per weight)."""
    nbytes = max(int(nbytes), 256)
    if nbytes < _ARENA_MIN_BYTES and not keep:
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    buf = _stream_buffer(_ARENA, device, nbytes, lambda n, dev: torch.empty(n, dtype=torch.uint8, device=dev))
    return buf[:nbytes]       # exactly what was asked for: some calls size their split-K slabs by the room they are given


def release_workspaces() -> None:
    """Drop the per-stream scratch buffers `_workspace` keeps (they return to torch's caching allocator)."""
    _ARENA.clear()
    _MINMAX_WS.clear()
    _RTN_STATE.clear()


def _rtn_state(nbytes: int, device) -> torch.Tensor | None:
    """The caller-kept state of `oq_rtn_quantize_stateful_f32`: zero before its first use and left zero by every call (the
    kernels clean up after themselves), so per-channel / per-tensor RTN needs no clear launch.  One buffer per (device,
    stream): calls on a stream run in order; at most four streams keep one.  A larger request takes a NEW zero-filled buffer."""
    if nbytes <= 0:
        return None
    return _stream_buffer(_RTN_STATE, device, nbytes, lambda n, dev: torch.zeros(max(int(n), 1 << 20), dtype=torch.uint8, device=dev))


def _row_major(t: torch.Tensor) -> tuple[torch.Tensor, int]:
    """Return (tensor, leading dimension) for a 2-D tensor whose rows are contiguous."""
    assert t.dim() == 2
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t, t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))


def _rows_and_out(x2: torch.Tensor, n: int, out_dtype):
    """The tail of a matmul front, for ``x2`` = x.reshape(-1, k): (x2 row-major as the C ABI wants it, m, lda, a fresh [m, n] out),
    or None where there are no rows (the front returns zeros and launches nothing)."""
    m = x2.shape[0]
    if m == 0:
        return None
    x2, lda = _row_major(x2)
    return x2, m, lda, torch.empty((m, n), dtype=out_dtype, device=x2.device)


def resolve_group(strategy: str, k: int, group_size) -> int:
    """Rows per (scale, zp): utils.py:16-22 for groups, K for channel / tensor."""
    if strategy != "group":
        return k
    g = min(group_size, k)
    return k if g == -1 else g


_HALF_WTYPE = {torch.float16: L.OQ_W_F16, torch.bfloat16: L.OQ_W_BF16}


def _twin(t: torch.Tensor) -> tuple:
    """For an entry point that exists as an `_f32` / `_h16` pair: the leading ``pointer[, type code]`` arguments for the
    operand ``t`` and the suffix of the name that takes them."""
    if t.dtype in _HALF_WTYPE:
        return (_ptr(t), _HALF_WTYPE[t.dtype]), "h16"
    return (_ptr(t),), "f32"


# the workspace queries of such pairs (their names are part of the ABI and follow no rule)
_TWIN_WORKSPACE = {
    "awq": {"f32": "oq_awq_workspace_bytes", "h16": "oq_awq_half_workspace_bytes"},
    "awq_stats": {"f32": "oq_awq_stats_workspace_bytes", "h16": "oq_awq_stats_half_workspace_bytes"},
    "absmax": {"f32": "oq_absmax_workspace_bytes", "h16": "oq_absmax_half_workspace_bytes"},
    "hessian": {"f32": "oq_hessian_workspace_bytes", "h16": "oq_hessian_half_workspace_bytes"},
    "hessian_many": {"f32": "oq_hessian_many_workspace_bytes", "h16": "oq_hessian_many_half_workspace_bytes"},
}


def _refuse_half(w, fn: str) -> None:
    """The entry points that stay fp32-only say so by name instead of a bare dtype mismatch."""
    if isinstance(w, torch.Tensor) and w.dtype in _HALF_WTYPE:
        raise TypeError(f"{fn} takes fp32 weights only, got {w.dtype}: half-precision weights are served by rtn_quantize "
                        f"(one matrix per call) and rtn_quantize_model (a list of matrices); convert with w.float() to use {fn}")


def _require_matrix(w, dtype=torch.float32) -> None:
    """``w`` is a 2-D device tensor (of ``dtype``, where one is given), or the error names what it is instead."""
    if not isinstance(w, torch.Tensor) or w.dim() != 2:
        _require_device(w, "w", dtype)
        raise ValueError(f"weights must be 2-D [K, N], got shape {tuple(w.shape)}")


def _rtn_param_shape(strategy: str, k: int, n: int, g: int):
    """(number of (scale, zp) pairs, the shape they are returned in) of a [K, N] matrix: rtn.py:98-109."""
    if strategy == "group":
        return (k * n) // g, ((k * n) // g, 1)
    if strategy == "channel":
        return n, (n,)
    return 1, ()


def _rtn_outputs(layout, k, n, g, qtype, count, dev, emit_q, out):
    """(q, scale, zp) of one matrix: the caller's ``out``, or new buffers (q None without ``emit_q``)."""
    if out is not None:
        return out
    q = _q_buffer(layout, (), k, n, g, qtype, dev) if emit_q else None
    return q, torch.empty(count, dtype=torch.float32, device=dev), torch.empty(count, dtype=container_dtype(qtype), device=dev)


def _rtn_quantize_half(w, qtype, strategy, group_size, symmetric, reduce_range, clip_ratio, layout, emit_q, out, mse=False):
    """`rtn_quantize` on an fp16 / bf16 matrix through oq_rtn_quantize_h16 (csrc/rtn_half.hip), or with ``mse`` (layout "kn"
    only, the caller's rule) through oq_rtn_mse_h16 (csrc/rtn_mse.hip): W is read as it is."""
    _require_matrix(w, None)
    _layout_code(layout)
    if layout == "kn_packed4":
        # no packed epilogue in the half kernels: the [K, N] route followed by the packer (the same bytes, core/_pack.py:8-22)
        if out is not None:
            raise ValueError("layout 'kn_packed4' of a half-precision matrix does not take `out`")
        if not emit_q:
            raise ValueError("layout 'kn_packed4' needs emit_q")
        k, n = w.shape
        g = resolve_group(strategy, k, group_size if group_size is not None else -1)
        if BITS[qtype] != 4 or n % 2 or strategy != "group" or g > 256:
            raise L.OqHipError(L.OQ_ERR_UNSUPPORTED, "KN_PACKED4 layout needs a 4-bit type, the group strategy with K % group_size == 0 "
                                                     "and group_size <= 256, and an even number of columns")
        q, scale, zp = _rtn_quantize_half(w, qtype, strategy, group_size, symmetric, reduce_range, clip_ratio, "kn", True, None)
        return pack_nibbles(q).reshape(k, n // 2), scale, zp
    w, ldw = _row_major(w)
    k, n = w.shape
    lib = L.load()
    g = resolve_group(strategy, k, group_size if group_size is not None else -1)
    count, shape = _rtn_param_shape(strategy, k, n, g)
    dev = w.device
    q, scale, zp = _rtn_outputs(layout, k, n, g, qtype, count, dev, emit_q, out)
    gs = -1 if group_size is None else int(group_size)
    # the two entry points take the same arguments
    query, entry = (lib.oq_rtn_mse_half_workspace_bytes, lib.oq_rtn_mse_h16) if mse else (lib.oq_rtn_half_workspace_bytes, lib.oq_rtn_quantize_h16)
    ws = _workspace(query(k, n, L.STRATEGY_CODE[strategy], gs), dev)
    L.check(entry(_ptr(w), _HALF_WTYPE[w.dtype], k, n, ldw, L.QTYPE_CODE[qtype], L.STRATEGY_CODE[strategy], gs,
                  int(symmetric), int(reduce_range), float(clip_ratio), _ptr(q if emit_q else None), _ptr(scale),
                  _ptr(zp), _layout_code(layout), _ptr(ws), ws.numel(), _stream()))
    return (q if emit_q else None), scale.reshape(shape), zp.reshape(shape)


# ----------------------------------------------------------------------------- A1 / Q2
def rtn_quantize(w: torch.Tensor, qtype: str, strategy: str, group_size=-1, symmetric=False,
                 reduce_range=False, clip_ratio=1.0, mse=False, layout: str = "kn", emit_q: bool = True,
                 out=None):
    """rtn.py:54-109 on the GPU.  ``w`` [K, N] fp32, fp16 or bf16 in HBM.

    Returns (q, scale, zp) -- q [K, N] (layout "kn"), the MatMulNBits blob [N, K/g, g*bits/8] (layout "nbits") or
    [K, N/2] nibble pairs in core/_pack.py:8-22 order (layout "kn_packed4": 4-bit types, group strategy);
    scale/zp 0-d | [N] | [N*K/g, 1].  With ``emit_q=False`` q is None
    (utils.py:302-348 only).

    A half-precision ``w`` gives, by definition, the result of this function on ``w.float()`` (both conversions are exact):
    the same integers, zero points and fp32 scales, bit for bit.  Its routes:
      - layouts "kn" / "nbits", any strategy, groups that divide K, no mse: oq_rtn_quantize_h16 reads the 2-byte matrix
        as it is (one fused launch for groups of up to 256 rows, a range pass and a quantize pass otherwise);
      - layout "kn_packed4": the "kn" route followed by `pack_nibbles`;
      - ``mse=True`` (layout "kn", groups that divide K): oq_rtn_mse_h16 runs the fp32 search's arithmetic on the 2-byte
        matrix, no fp32 copy; a group of 256 is held in registers as packed halves, which the fp32 search cannot do;
      - groups that straddle columns (K % group_size != 0) have no half kernel: ONE device cast, ``w.float()``, then the
        fp32 path below (``mse=True`` with a layout other than "kn" goes there too, for the fp32 path's refusal).
    A LIST of half matrices (a resident model) goes through `rtn_quantize_model`: one launch for the matrices of a shape.
    """
    _require_device(w, "w")
    if w.dtype in _HALF_WTYPE:
        if w.dim() == 2:
            g_h = resolve_group(strategy, w.shape[0], group_size if group_size is not None else -1)
            if g_h > 0 and w.shape[0] % g_h == 0 and (not mse or layout == "kn"):
                return _rtn_quantize_half(w, qtype, strategy, group_size, symmetric, reduce_range, clip_ratio, layout, emit_q, out, mse)
        w = w.float()      # the documented cast route: straddling groups (and mse with a layout it refuses: the fp32 path's error)
    _require_device(w, "w", torch.float32)
    _require_matrix(w)
    w, ldw = _row_major(w)
    k, n = w.shape
    lib = L.load()
    g = resolve_group(strategy, k, group_size if group_size is not None else -1)
    if strategy == "group" and (g <= 0 or (k * n) % g):
        raise ValueError(f"cannot reshape array of size {k * n} into shape (-1, {g})")
    count, shape = _rtn_param_shape(strategy, k, n, g)
    dev = w.device
    q, scale, zp = _rtn_outputs(layout, k, n, g, qtype, count, dev, emit_q, out)
    gs = -1 if group_size is None else int(group_size)
    ws_bytes = lib.oq_rtn_workspace_bytes(k, n, L.STRATEGY_CODE[strategy], gs, int(mse))
    ws = _workspace(ws_bytes, dev)
    if emit_q:
        state = None if mse else _rtn_state(lib.oq_rtn_state_bytes(k, n, L.STRATEGY_CODE[strategy], gs), dev)
        st = lib.oq_rtn_quantize_stateful_f32(_ptr(w), k, n, ldw, L.QTYPE_CODE[qtype], L.STRATEGY_CODE[strategy], gs,
                                              int(symmetric), int(reduce_range), float(clip_ratio), int(mse), _ptr(q),
                                              _ptr(scale), _ptr(zp), _layout_code(layout),
                                              _ptr(ws), ws.numel(), _ptr(state), 0 if state is None else state.numel(), _stream())
    else:
        st = lib.oq_rtn_qparams_f32(_ptr(w), k, n, ldw, L.QTYPE_CODE[qtype], L.STRATEGY_CODE[strategy], gs,
                                    int(symmetric), int(reduce_range), float(clip_ratio), int(mse), _ptr(scale),
                                    _ptr(zp), _ptr(ws), ws.numel(), _stream())
    L.check(st)
    return q, scale.reshape(shape), zp.reshape(shape)


def fingerprint64(t: torch.Tensor) -> int:
    """64-bit content fingerprint of a contiguous device tensor's bytes (`oq_fingerprint64`, one pass at the HBM rate).  Synchronises
    (eight bytes come back): it decides what the host does next (seam.py: reuse a cached Hessian or compute it)."""
    _require_device(t, "t")
    if not t.is_contiguous():
        raise ValueError("fingerprint64 needs a contiguous tensor")
    nbytes = t.numel() * t.element_size()
    if nbytes == 0:
        raise ValueError("fingerprint64 of an empty tensor")
    if t.data_ptr() % 16:
        t = t.clone()
    out = torch.empty(1, dtype=torch.int64, device=t.device)
    L.check(L.load().oq_fingerprint64(_ptr(t), nbytes, _ptr(out), _stream()))
    return int(out.item()) & 0xFFFFFFFFFFFFFFFF


def hqq_quantize(w: torch.Tensor, group_size: int, reduce_range=False, clip_ratio=1.0, mse=False, lp_norm=0.7, beta=1e1,
                 kappa=1.01, iters=20, early_stop=True, emit_q: bool = True, layout: str = "kn", per_round_launches: bool = False):
    """hqq.py:147-213 on the GPU: uint4 / asymmetric / group with float zero points.  ``w`` [K, N] fp32, fp16 or bf16 in HBM.
    Returns (q [K, N] uint8 | MatMulNBits blob [N, K/g, g/2] for layout="nbits" | None, scale [N*K/g, 1] fp32,
    zero_point [N*K/g, 1] fp32, rounds int32[1] on device).

    A half-precision ``w`` gives, by definition, the result of this function on ``w.float()`` (both conversions are exact, the
    arithmetic of HQQ stays fp32): the same integers, scales, zero points and rounds, bit for bit.  oq_hqq_optimize_h16 reads the
    2-byte matrix as it is, rows that are only 2-byte aligned included; no fp32 copy exists.  The initial parameters come from
    `rtn_quantize` on the half matrix, with ``mse=True`` from its half MSE search (oq_rtn_mse_h16): no route makes an fp32
    copy.  A group of 256 runs all rounds in one pass over a half ``w``
    (the fp32 kernels re-read W every round at that size); ``per_round_launches=True`` forces the per-round route."""
    _require_device(w, "w")
    if w.dtype not in _HALF_WTYPE:
        _require_device(w, "w", torch.float32)
    if w.dim() != 2:
        raise ValueError(f"weights must be 2-D [K, N], got shape {tuple(w.shape)}")
    w, ldw = _row_major(w)
    k, n = w.shape
    g = resolve_group("group", k, group_size if group_size is not None else -1)
    if g <= 0 or (k * n) % g:
        raise ValueError(f"cannot reshape array of size {k * n} into shape (-1, {g})")
    # hqq.py:181-192: initial parameters = the RTN ones with float zero points (integral values)
    _, scale, zp0 = rtn_quantize(w, "uint4", "group", group_size, False, reduce_range, clip_ratio, mse, emit_q=False)
    lib = L.load()
    dev = w.device
    rows = (k * n) // g
    zp_in = zp0.reshape(-1).to(torch.float32)
    zp = torch.empty(rows, dtype=torch.float32, device=dev)
    if not emit_q:
        q = None
    elif layout == "kn":
        q = torch.empty((k, n), dtype=torch.uint8, device=dev)
    else:
        q = torch.empty((n, k // g, g // 2), dtype=torch.uint8, device=dev)
    rounds = torch.zeros(1, dtype=torch.int32, device=dev)
    gs = -1 if group_size is None else int(group_size)
    ws = _workspace(lib.oq_hqq_workspace_bytes(k, n, gs), dev, keep=True)
    wargs, kind = _twin(w)
    L.check(getattr(lib, "oq_hqq_optimize_" + kind)(*wargs, k, n, ldw, gs, int(reduce_range), _ptr(scale), _ptr(zp_in), float(lp_norm), float(beta),
                                                    float(kappa), int(iters), int(early_stop), int(bool(per_round_launches)), _ptr(q),
                                                    L.OQ_LAYOUT_KN if layout == "kn" else L.OQ_LAYOUT_NBITS, _ptr(zp), _ptr(rounds), _ptr(ws),
                                                    ws.numel(), _stream()))
    return q, scale.reshape(rows, 1), zp.reshape(rows, 1), rounds


def rtn_quantize_tensor_many(ws, qtype: str, symmetric=False, reduce_range=False, clip_ratio=1.0):
    """rtn.py:54-109 with strategy "tensor" for a list of contiguous fp32 weights of any shapes in THREE launches
    (oq_rtn_tensor_many_f32): a model of many small matrices makes a per-matrix loop launch-bound.  4- / 8-bit types.
    Returns [(q like w in the container dtype, scale 0-d fp32, zp 0-d)], views of three shared buffers."""
    if not ws:
        return []
    if BITS[qtype] > 8:
        raise NotImplementedError("rtn_quantize_tensor_many: 4- and 8-bit types only")
    flats = []
    for w in ws:
        _refuse_half(w, "rtn_quantize_tensor_many")
        _require_device(w, "w", torch.float32)
        flats.append(w if w.is_contiguous() else w.contiguous())
    dev = flats[0].device
    cdt = container_dtype(qtype)
    counts = [f.numel() for f in flats]
    if min(counts) == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + (c + 15) // 16 * 16)                 # every q slice starts 16-byte aligned
    q_all = torch.empty(offs[-1], dtype=cdt, device=dev)
    s_all = torch.empty(len(flats), dtype=torch.float32, device=dev)
    z_all = torch.empty(len(flats), dtype=cdt, device=dev)
    qb, sb, zb = q_all.data_ptr(), s_all.data_ptr(), z_all.data_ptr()
    _, _, table = _item_table([[f.data_ptr(), c, qb + o, sb + 4 * i, zb + i] for i, (f, c, o) in enumerate(zip(flats, counts, offs))], dev)
    lib = L.load()
    wsb = _workspace(lib.oq_rtn_tensor_many_workspace_bytes(len(flats)), dev)
    L.check(lib.oq_rtn_tensor_many_f32(_ptr(table), len(flats), L.QTYPE_CODE[qtype], int(symmetric), int(reduce_range),
                                       float(clip_ratio), _ptr(wsb), wsb.numel(), _stream()))
    return [(q_all[o:o + c].view(f.shape), s_all[i], z_all[i]) for i, (f, c, o) in enumerate(zip(flats, counts, offs))]


def rtn_quantize_batched(w: torch.Tensor, qtype: str, group_size: int, symmetric=False, reduce_range=False,
                         clip_ratio=1.0, layout: str = "kn", out=None):
    """rtn.py:54-109 for a stack of equally shaped weights ``w`` [B, K, N] in ONE launch (group strategy).
    Returns (q [B, K, N] | [B, N, K/g, g*bits/8], scale [B, N*K/g, 1], zp [B, N*K/g, 1])."""
    _refuse_half(w, "rtn_quantize_batched")
    _require_device(w, "w", torch.float32)
    if w.dim() != 3 or not w.is_contiguous():
        raise ValueError("w must be a contiguous [B, K, N] tensor")
    b, k, n = w.shape
    g = resolve_group("group", k, group_size)
    if k % g:
        raise ValueError("batched RTN needs K % group_size == 0")
    lib = L.load()
    cdt = container_dtype(qtype)
    if out is not None:
        q, scale, zp = out
    else:
        q = _q_buffer(layout, (b,), k, n, g, qtype, w.device)
        scale = torch.empty((b, n * k // g, 1), dtype=torch.float32, device=w.device)
        zp = torch.empty((b, n * k // g, 1), dtype=cdt, device=w.device)
    ws = _workspace(lib.oq_rtn_batched_workspace_bytes(b, k, n, int(group_size)), w.device)
    L.check(lib.oq_rtn_quantize_batched_f32(_ptr(w), b, k * n, k, n, n, L.QTYPE_CODE[qtype], int(group_size), int(symmetric),
                                            int(reduce_range), float(clip_ratio), _ptr(q), _ptr(scale), _ptr(zp),
                                            _layout_code(layout), _ptr(ws), ws.numel(), _stream()))
    return q, scale, zp


_TABLE_STAGE: dict = {}     # device index -> (pinned int64 [cap, 4], side stream): the pointer tables of rtn_quantize_many


def _table_stage(dev, rows: int):
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    pin, side = _TABLE_STAGE.get(index, (None, None))
    if side is None:
        side = torch.cuda.Stream(device=dev)
    if pin is None or pin.shape[0] < rows:
        pin = torch.empty((max(rows, 256), 4), dtype=torch.int64).pin_memory()
    _TABLE_STAGE[index] = (pin, side)
    side.synchronize()          # an earlier call's copies have left the pinned rows (they ran long ago: this returns at once)
    return pin, side


def _table_rows(layout: str, cnt: int, k: int, n: int, g: int, qtype: str, dev, w_ptrs, pin_np, row: int):
    """One C call of a pointer-table entry point (oq_rtn_ptrs / oq_rtn_ptrs_h16: {W, q_out, scale_out, zp_out}): allocate the
    stacked outputs of its ``cnt`` matrices of one shape and write rows [row, row + cnt) of the page-locked table (host side
    only).  Returns (q, scale, zp) with the matrix as the leading dimension."""
    q = _q_buffer(layout, (cnt,), k, n, g, qtype, dev)
    sc = torch.empty((cnt, n * k // g, 1), dtype=torch.float32, device=dev)
    zp = torch.empty((cnt, n * k // g, 1), dtype=container_dtype(qtype), device=dev)
    # output pointers by arithmetic (the per-matrix views the caller gets back are made AFTER the launches)
    rows = pin_np[row:row + cnt]
    steps = np.arange(cnt, dtype=np.int64)
    rows[:, 0] = w_ptrs
    rows[:, 1] = q.data_ptr() + steps * (q[0].numel() * q.element_size())
    rows[:, 2] = sc.data_ptr() + steps * (sc[0].numel() * 4)
    rows[:, 3] = zp.data_ptr() + steps * (zp[0].numel() * zp.element_size())
    return q, sc, zp


def _upload_rows(pin, table_dev, side, row: int, cnt: int) -> None:
    """Rows [row, row + cnt) of the table to the device on the side stream; the launch stream waits for them."""
    cur = torch.cuda.current_stream()
    with torch.cuda.stream(side):
        table_dev[row:row + cnt].copy_(pin[row:row + cnt], non_blocking=True)
        ready = side.record_event()
    cur.wait_event(ready)


def rtn_quantize_many(ws, qtype: str, group_size: int, symmetric=False, reduce_range=False, clip_ratio=1.0, layout: str = "kn"):
    """rtn.py:54-109 (group strategy) for a LIST of [K, N] fp32 weights of any shapes living anywhere in HBM -- the MatMul
    weights of a model, which the reference quantizes node by node (qrules/_common.py:126-142).  Weights of one shape go
    through ONE C call (oq_rtn_quantize_ptrs_f32), which puts about 1.6e8 parameters into a launch (a device table of
    pointers, blockIdx.y = entry): rounds of waves merge across matrices and small matrices are no longer launch-bound
    (gemma-3-270m's 126 weights: 1.0 ms instead of 2.6 ms in a per-matrix loop; 4096 x 4096 at a model's footprint: 0.72 of
    the HBM peak instead of 0.54).  Per matrix the bits are those of `rtn_quantize`.  Returns [(q, scale, zp)] in input order; q [K, N], the
    MatMulNBits blob [N, K/g, g*bits/8] or [K, N/2] nibble pairs (layout "kn_packed4"), scale / zp [N*K/g, 1]; the outputs of
    one C call (a shape, or a piece of the first shapes) are views of three shared buffers.

    Host work runs beside the kernels (see the comments in the body): the pointer tables go through a page-locked staging
    buffer and a side stream, and the calls are ordered and cut so that only ~50 us of head have the GPU waiting (with all
    tables built and uploaded before the first launch a 224-matrix model had 0.4 ms of idle GPU in front of 5.7 ms of
    kernels; a blocking upload per shape on the launch stream was worse: it queues behind the previous shape's kernels)."""
    if not ws:
        return []
    lib = L.load()
    lay = _layout_code(layout)

    def by_shape(indices):
        """The weights at ``indices`` by (shape, strides): the members of one C call."""
        groups: dict = {}
        for i in indices:
            w = ws[i]
            if not isinstance(w, torch.Tensor) or w.dim() != 2:     # tested here: no helper call per weight on the way that passes
                _require_matrix(w)
            # two attribute reads per weight: the scan of 224 weights is 0.1 ms of head otherwise
            groups.setdefault((w.shape, w.stride()), []).append(i)
        return groups

    dev = ws[0].device
    out = [None] * len(ws)
    pin, side = _table_stage(dev, len(ws))
    table_dev = torch.empty((len(ws), 4), dtype=torch.int64, device=dev)
    table_dev.record_stream(side)
    state = {"wsb": None, "row": 0}
    made = []

    pin_np = pin.numpy()                       # the page-locked rows as a NumPy view: filling them costs microseconds, not torch dispatches
    cur_dev = torch.cuda.current_device()

    def prepare(key, idx):
        """Check the members of one C call, allocate their outputs, write their table rows (host side only)."""
        (k, n), _strides = key
        if k == 0 or n == 0:
            raise ValueError(f"rtn_quantize_many: weight {idx[0]} is empty ({k} x {n})")
        g = resolve_group("group", k, group_size)
        if g <= 0 or k % g:
            raise ValueError("rtn_quantize_many needs K % group_size == 0 for every weight")
        mats, ldw = [], None
        st0 = _strides[0]                         # every member of a call shares shape and strides (the grouping key)
        plain = _strides[1] == 1 and st0 >= n and k > 1
        for i in idx:
            w = ws[i]
            if not (w.is_cuda and w.dtype is torch.float32 and w.device.index == cur_dev):
                _refuse_half(w, "rtn_quantize_many")
                _require_device(w, "w", torch.float32)      # raises with the full message
            if plain:                              # rows contiguous: the tensor as it is (the per-weight helper calls were a third of
                w2, ldw = w, st0                   # this function's time on a 126-weight model)
            else:
                w2, ldw = _row_major(w)
            mats.append(w2)
        cnt, row = len(idx), state["row"]
        q, sc, zp = _table_rows(layout, cnt, k, n, g, qtype, dev, [m.data_ptr() for m in mats], pin_np, row)
        need = lib.oq_rtn_batched_workspace_bytes(cnt, k, n, int(group_size))
        if state["wsb"] is None or state["wsb"].numel() < need:
            state["wsb"] = _workspace(need, dev)     # calls on one stream run in order: a later, larger shape may take a new buffer
        made.append((idx, q, sc, zp, mats))      # operands stay referenced until the views are made
        state["row"] = row + cnt
        return (k, n, ldw, cnt, row, state["wsb"])

    def launch(call):
        k, n, ldw, cnt, row, wsb = call
        L.check(lib.oq_rtn_quantize_ptrs_f32(C.c_void_p(pin[row:row + cnt].data_ptr()), C.c_void_p(table_dev[row:row + cnt].data_ptr() if cnt > 1 else 0), cnt,
                                             k, n, ldw, L.QTYPE_CODE[qtype], int(group_size), int(symmetric), int(reduce_range), float(clip_ratio), lay,
                                             _ptr(wsb), wsb.numel(), _stream()))

    def run(key, idx):
        """One C call: prepare, copy its table rows, launch."""
        call = prepare(key, idx)
        if call[3] > 1:
            _upload_rows(pin, table_dev, side, call[4], call[3])
        launch(call)

    def views():
        for idx, q, sc, zp, _mats in made:
            for j, i in enumerate(idx):
                out[i] = (q[j], sc[j], zp[j])
        return out

    # Host work beside the kernels.  (1) Look at the first 24 weights only and launch up to 8 of the shape that carries the
    # most parameters among them: the GPU starts after ~50 us of head.  (2) Group everything else by shape while those
    # kernels run.  (3) Shape by shape, fewest matrices first; the first shape in pieces (4, 8, rest) so that every call is
    # prepared in less time than the kernels in front of it take.
    # A small model (gemma-3-270m: 126 weights, 1e8 parameters, 0.2 ms of kernels) is bound by this function, not by its kernels:
    # everything is prepared first, the table goes up in ONE copy and the C calls follow back to back (0.90 -> see the bench's
    # `model_rtn.small_matrices`).  The interleaving below pays from a few hundred million parameters on.
    if sum(w.shape[0] * w.shape[1] for w in ws if isinstance(w, torch.Tensor) and w.dim() == 2) < (1 << 29):
        calls = [prepare(key, idx) for key, idx in by_shape(range(len(ws))).items()]
        if any(c[3] > 1 for c in calls):
            _upload_rows(pin, table_dev, side, 0, state["row"])
        for c in calls:
            launch(c)
        return views()
    taken = set()
    if len(ws) > 24:
        key0, idx0 = max(by_shape(range(24)).items(), key=lambda kv: len(kv[1]) * kv[0][0][0] * kv[0][0][1])
        run(key0, idx0[:8])
        taken = set(idx0[:8])
    order = sorted(by_shape([i for i in range(len(ws)) if i not in taken]).items(), key=lambda kv: len(kv[1]))
    if order and len(order[0][1]) > 12:
        key1, idx1 = order[0]
        order = [(key1, idx1[:4]), (key1, idx1[4:12]), (key1, idx1[12:])] + order[1:]
    for key, idx in order:
        run(key, idx)
    return views()


_HALF_WAVE_GROUPS = (16, 32, 64, 128, 256)     # csrc/rtn_half.hip: the group sizes rtn_half_wave has a build for


def _half_list_route(w, g: int, qtype: str, layout: str) -> bool:
    """Whether oq_rtn_quantize_ptrs_h16 takes this half matrix as it is (rows contiguous, a group the fused kernels hold, a
    layout the kernel of that group writes, per-matrix outputs that stay aligned inside a shared buffer)."""
    k, n = w.shape
    if g > 256 or w.stride(1) != 1 or (k > 1 and w.stride(0) < n):
        return False
    if layout == "kn_packed4":
        return g in _HALF_WAVE_GROUPS and BITS[qtype] == 4 and n % 2 == 0
    if layout == "nbits":
        return g % 16 == 0 and (n * k * BITS[qtype] // 8) % 16 == 0
    return True


def rtn_quantize_model(ws, qtype: str, group_size: int, symmetric=False, reduce_range=False, clip_ratio=1.0, layout: str = "kn"):
    """rtn.py:54-109 (group strategy) for the MatMul weights of a model resident in HBM: a LIST of [K, N] device weights of any
    mix of fp32 / fp16 / bf16 and of any shapes.  Returns [(q, scale, zp)] in input order with the shapes and dtypes of
    `rtn_quantize_many`; per matrix the bits are those of `rtn_quantize` on that tensor (for a half tensor: on its upcast).

      - fp32 items go to `rtn_quantize_many`, unchanged;
      - half items are grouped by (dtype, shape, strides, 16-byte alignment of the base) and every group is ONE
        oq_rtn_quantize_ptrs_h16 call (csrc/rtn_half.hip: the fused half kernels with blockIdx.y = entry of a device table of
        pointers; no fp32 copy, no workspace): a tensor viewed from an odd offset never puts the aligned ones on the narrow loads.
        Layout "kn_packed4" comes straight out of that launch (no [K, N] intermediate, no packer);
      - half items that entry point does not take -- groups taller than 256 rows, the packed layout on a group size without a
        wave build, rows that are not contiguous -- go one by one through `rtn_quantize`.

    The outputs of one C call are views of three shared buffers.  All table rows go through the page-locked staging rows and
    the side stream of `rtn_quantize_many`'s small-model path: everything is prepared first, the table goes up in one copy and
    the C calls follow back to back."""
    if not ws:
        return []
    lay = _layout_code(layout)
    out = [None] * len(ws)
    here = torch.device("cuda", torch.cuda.current_device())
    f32, singles = [], []
    groups: dict = {}       # (dtype, shape, strides, base 16-byte aligned) -> [takes the list route, indices, W pointers]
    for i, w in enumerate(ws):              # a handful of attribute reads per weight: a small model is bound by this function
        dt = getattr(w, "dtype", None)
        if dt not in _HALF_WTYPE:
            f32.append(i)                   # rtn_quantize_many checks (and names) what is not an fp32 device tensor
            continue
        if w.device != here:
            _require_device(w, "w")         # raises with the full message
        ptr = w.data_ptr()
        key = (dt, w.shape, w.stride(), (ptr & 15) == 0)
        slot = groups.get(key)
        if slot is None:                    # the first of its key: the checks every member shares
            _require_matrix(w, None)
            k, n = w.shape
            if k == 0 or n == 0:
                raise ValueError(f"rtn_quantize_model: weight {i} is empty ({k} x {n})")
            g = resolve_group("group", k, group_size)
            if g <= 0 or k % g:
                raise ValueError("rtn_quantize_model needs K % group_size == 0 for every weight")
            slot = groups[key] = [_half_list_route(w, g, qtype, layout), [], []]
        slot[1].append(i)
        slot[2].append(ptr)
    for key in [key for key, slot in groups.items() if not slot[0]]:
        singles.extend(groups.pop(key)[1])
    if f32:
        for i, r in zip(f32, rtn_quantize_many([ws[i] for i in f32], qtype, group_size, symmetric, reduce_range, clip_ratio, layout)):
            out[i] = r
    if groups:
        lib = L.load()
        total = sum(len(slot[1]) for slot in groups.values())
        pin, side = _table_stage(here, total)
        table_dev = torch.empty((total, 4), dtype=torch.int64, device=here)
        table_dev.record_stream(side)
        pin_np = pin.numpy()
        calls, made, row = [], [], 0
        for (dtype, (k, n), strides, _aligned), (_ok, idx, ptrs) in groups.items():     # host side only: outputs and table rows of every call
            cnt = len(idx)
            q, sc, zp = _table_rows(layout, cnt, k, n, resolve_group("group", k, group_size), qtype, here, ptrs, pin_np, row)
            calls.append((_HALF_WTYPE[dtype], k, n, strides[0] if k > 1 else max(n, strides[0]), cnt, row))
            made.append((idx, q, sc, zp))
            row += cnt
        if any(c[4] > 1 for c in calls):           # one copy for every call
            _upload_rows(pin, table_dev, side, 0, total)
        host0, dev0, stream = pin.data_ptr(), table_dev.data_ptr(), _stream()
        for wtype, k, n, ldw, cnt, row in calls:
            L.check(lib.oq_rtn_quantize_ptrs_h16(C.c_void_p(host0 + 32 * row), C.c_void_p(dev0 + 32 * row if cnt > 1 else 0), cnt, wtype, k, n, ldw,
                                                 L.QTYPE_CODE[qtype], int(group_size), int(symmetric), int(reduce_range), float(clip_ratio), lay, stream))
        for idx, q, sc, zp in made:                # the per-matrix views, one unbind per buffer
            for i, r in zip(idx, zip(q.unbind(0), sc.unbind(0), zp.unbind(0))):
                out[i] = r
    for i in singles:
        out[i] = rtn_quantize(ws[i], qtype, "group", group_size, symmetric, reduce_range, clip_ratio, layout=layout)
    return out


# ----------------------------------------------------------------------------- Q1
def qparams(rmin: torch.Tensor, rmax: torch.Tensor, qtype: str, symmetric: bool, reduce_range: bool):
    """utils.py:242-299 on device ranges (any shape); returns (scale fp32, zp int32) of that shape."""
    _require_device(rmin, "rmin", torch.float32)
    _require_device(rmax, "rmax", torch.float32)
    a, b = rmin.contiguous().reshape(-1), rmax.contiguous().reshape(-1)
    scale = torch.empty_like(a)
    zp = torch.empty(a.numel(), dtype=torch.int32, device=a.device)
    L.check(L.load().oq_qparams_f32(_ptr(a), _ptr(b), a.numel(), L.QTYPE_CODE[qtype], int(symmetric),
                                    int(reduce_range), _ptr(scale), _ptr(zp), _stream()))
    return scale.reshape(rmin.shape), zp.reshape(rmin.shape)


def qparams_f64(rmin: torch.Tensor, rmax: torch.Tensor, qtype: str, symmetric: bool, reduce_range: bool):
    """utils.py:242-299 for float64 ranges (arithmetic in double, fp32 scale out)."""
    _require_device(rmin, "rmin", torch.float64)
    _require_device(rmax, "rmax", torch.float64)
    a, b = rmin.contiguous().reshape(-1), rmax.contiguous().reshape(-1)
    scale = torch.empty(a.numel(), dtype=torch.float32, device=a.device)
    zp = torch.empty(a.numel(), dtype=torch.int32, device=a.device)
    L.check(L.load().oq_qparams_f64(_ptr(a), _ptr(b), a.numel(), L.QTYPE_CODE[qtype], int(symmetric),
                                    int(reduce_range), _ptr(scale), _ptr(zp), _stream()))
    return scale.reshape(rmin.shape), zp.reshape(rmin.shape)


def minmax_rows(x: torch.Tensor):
    """utils.py:60-61 (axis=1): raw per-row (min, max) of a 2-D fp32 tensor."""
    _require_device(x, "x", torch.float32)
    x2, ldx = _row_major(x)
    r, c = x2.shape
    mn = torch.empty(r, dtype=torch.float32, device=x.device)
    mx = torch.empty(r, dtype=torch.float32, device=x.device)
    L.check(L.load().oq_minmax_rows_f32(_ptr(x2), r, c, ldx, _ptr(mn), _ptr(mx), _stream()))
    return mn, mx


# ----------------------------------------------------------------------------- K1 / K2
def _param_index(mode: str, r: int, c: int, group: int = 1):
    if mode == "tensor":
        return 1, 0, 0
    if mode == "row":
        return 1, 1, 0
    if mode == "col":
        return 1, 0, 1
    if mode == "group":        # groups of `group` rows on a [K, N] matrix, entry n*(K/g)+kg
        return group, 1, r // group
    raise ValueError(mode)


def _ragged_group(r: int, c: int, mode: str, group: int) -> bool:
    """Groups of `group` rows that do not divide K: the reference then forms them on `W.T.reshape(-1, g)` (utils.py:24),
    i.e. element (k, n) belongs to group (n*K + k) // g and groups straddle columns."""
    if mode != "group" or r % group == 0:
        return False
    if (r * c) % group:
        raise ValueError(f"cannot reshape array of size {r * c} into shape (-1, {group})")
    return True


def _zero_point_words(zp: torch.Tensor) -> torch.Tensor:
    """Integer zero points as the flat 32-bit words of oq_quantize_f32 / oq_dequantize_f32 (include/oq_hip.h: read as unsigned
    for uint32, signed otherwise).  A `torch.uint32` tensor hands over its bits; the other integer dtypes are narrowed to
    32 bits, which keeps the bits of every value of either reading, so a uint32 zero point of 2^31 or more held in an int64
    tensor arrives intact as well.  Values are not inspected (that would synchronise): they are the caller's contract."""
    if zp.dtype == torch.uint32:
        return zp.contiguous().reshape(-1).view(torch.int32)
    return zp.to(torch.int32).contiguous().reshape(-1)


def quantize(x: torch.Tensor, scale: torch.Tensor, zp: torch.Tensor, qtype: str, symmetric: bool,
             reduce_range: bool, mode: str = "tensor", group: int = 1) -> torch.Tensor:
    """utils.py:72-79.  x [R, C] fp32; (scale, zp) indexed per `mode` (see oq_quantize_f32)."""
    _require_device(x, "x", torch.float32)
    x2 = x.reshape(1, -1) if x.dim() != 2 else x
    if _ragged_group(x2.shape[0], x2.shape[1], mode, group):      # the reference's own row layout, one parameter per row
        rows = x2.t().contiguous().reshape(-1, group)
        return quantize(rows, scale, zp, qtype, symmetric, reduce_range, mode="row").reshape(x2.shape[1], x2.shape[0]).t().contiguous()
    x2, ldx = _row_major(x2)
    r, c = x2.shape
    s = scale.to(torch.float32).contiguous().reshape(-1)
    z = _zero_point_words(zp)
    q = torch.empty((r, c), dtype=container_dtype(qtype), device=x.device)
    rd, rs, cs = _param_index(mode, r, c, group)
    L.check(L.load().oq_quantize_f32(_ptr(x2), r, c, ldx, _ptr(s), _ptr(z), rd, rs, cs, L.QTYPE_CODE[qtype],
                                     int(symmetric), int(reduce_range), _ptr(q), _stream()))
    return q.reshape(x.shape)


def dequantize(q: torch.Tensor, scale: torch.Tensor, zp: torch.Tensor, qtype: str, mode: str = "tensor",
               group: int = 1) -> torch.Tensor:
    """utils.py:102-137 (without the layout shuffles: `mode` addresses the parameters in place).  Floating-point zero
    points (HQQ, hqq.py:77-78) are subtracted as they are, like `zero_point.astype(float32)` in utils.py:131."""
    _require_device(q, "q", container_dtype(qtype))
    q2 = q.reshape(1, -1) if q.dim() != 2 else q
    if _ragged_group(q2.shape[0], q2.shape[1], mode, group):
        rows = q2.t().contiguous().reshape(-1, group)
        return dequantize(rows, scale, zp, qtype, mode="row").reshape(q2.shape[1], q2.shape[0]).t().contiguous()
    q2 = q2.contiguous()
    r, c = q2.shape
    s = scale.to(torch.float32).contiguous().reshape(-1)
    out = torch.empty((r, c), dtype=torch.float32, device=q.device)
    rd, rs, cs = _param_index(mode, r, c, group)
    if zp.dtype.is_floating_point:
        z = zp.to(torch.float32).contiguous().reshape(-1)
        L.check(L.load().oq_dequantize_fzp_f32(_ptr(q2), r, c, L.QTYPE_CODE[qtype], _ptr(s), _ptr(z), rd, rs, cs,
                                               _ptr(out), c, _stream()))
    else:
        z = _zero_point_words(zp)
        L.check(L.load().oq_dequantize_f32(_ptr(q2), r, c, L.QTYPE_CODE[qtype], _ptr(s), _ptr(z), rd, rs, cs,
                                           _ptr(out), c, _stream()))
    return out.reshape(q.shape)


def quantize_bias(bias: torch.Tensor, x_scale: float, w_scale: torch.Tensor):
    """rtn.py:112-138 -> (int32 bias, fp32 bias scale)."""
    _require_device(bias, "bias", torch.float32)
    _require_device(w_scale, "weight_scale", torch.float32)
    b = bias.contiguous()
    ws = w_scale.contiguous().reshape(-1)
    q = torch.empty(b.numel(), dtype=torch.int32, device=b.device)
    bs = torch.empty(b.numel(), dtype=torch.float32, device=b.device)
    L.check(L.load().oq_quantize_bias_f32(_ptr(b), b.numel(), _ptr(ws), ws.numel(), float(x_scale), _ptr(q),
                                          _ptr(bs), _stream()))
    return q, bs


# ----------------------------------------------------------------------------- C1 / S1
def minmax_state(device, dtype=torch.float32) -> torch.Tensor:
    """Fresh device-resident calibrator state {min, max, seen, -} (see oq_minmax_collect_f32)."""
    return torch.zeros(4, dtype=dtype, device=device)


def minmax_collect(x: torch.Tensor, state: torch.Tensor, momentum: float = 0.0) -> None:
    """minmax.py:40-64: fold one activation batch into `state`, entirely on the device.  This sits in the
    calibration loop (thousands of tensors per run), so the host side is kept to one ctypes call.

    An fp16 / bf16 ``x`` is read as it is (`oq_minmax_collect_h16`, csrc/reduce_half.hip) into an fp32 state: the state of
    the fp32 call on ``x.float()``, bit for bit, without that copy."""
    half = x.dtype in _HALF_WTYPE
    if not x.is_cuda or not (half or x.dtype in (torch.float32, torch.float64)):
        raise TypeError("activations must be fp32/fp64 tensors in GPU memory")
    if half:
        if state.dtype != torch.float32:
            raise TypeError(f"the state of an {x.dtype} activation must be fp32, got {state.dtype}")
    elif state.dtype != x.dtype:
        raise TypeError("state dtype must match the activation dtype")
    flat = x if x.is_contiguous() else x.contiguous()
    n = flat.numel()
    if n == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    lib = L.load()
    stream = torch.cuda.current_stream(x.device).cuda_stream
    ws = _MINMAX_WS.get((x.device.index, stream))      # a hit costs this lookup and no more: it does not move the entry to the end
    if ws is None:    # one workspace serves both entry points (neither size depends on the count)
        ws = _stream_buffer(_MINMAX_WS, x.device, max(lib.oq_minmax_workspace_bytes(n), lib.oq_minmax_half_workspace_bytes(n)), _workspace)
    if half:
        st = lib.oq_minmax_collect_h16(flat.data_ptr(), _HALF_WTYPE[x.dtype], n, state.data_ptr(), float(momentum), ws.data_ptr(),
                                       ws.numel(), stream)
    else:
        fn = lib.oq_minmax_collect_f32 if x.dtype == torch.float32 else lib.oq_minmax_collect_f64
        st = fn(flat.data_ptr(), n, state.data_ptr(), float(momentum), ws.data_ptr(), ws.numel(), stream)
    if st:
        L.check(st)


def minmax_collect_many(xs, states, momentum: float = 0.0) -> None:
    """minmax.py:40-64 for a list of tensors of ONE dtype -- fp32 (oq_minmax_collect_many_f32), fp16 or bf16
    (oq_minmax_collect_many_h16, read as they are) -- in ONE launch pair: ``xs[i]`` is folded into the fp32 ``states[i]``.
    The 24-byte descriptors travel in one small host-to-device copy per call."""
    if len(xs) != len(states) or not xs:
        raise ValueError("minmax_collect_many needs equally long, non-empty lists")
    dtype = xs[0].dtype if xs[0].dtype in _HALF_WTYPE else torch.float32
    flats = []
    for x, st in zip(xs, states):
        if not x.is_cuda or x.dtype != dtype or st.dtype != torch.float32:
            if dtype != torch.float32 and x.is_cuda and x.dtype in (torch.float32, *_HALF_WTYPE) and st.dtype == torch.float32:
                raise TypeError(f"minmax_collect_many takes tensors of one dtype per call, got {dtype} and {x.dtype}")
            raise TypeError("minmax_collect_many takes fp32 tensors in GPU memory (use minmax_collect for fp64)")
        f = x if x.is_contiguous() else x.contiguous()
        if f.numel() == 0:
            raise ValueError("zero-size array to reduction operation minimum which has no identity")
        flats.append(f)
    dev = flats[0].device
    _, _, desc = _item_table([[f.data_ptr(), f.numel(), st.data_ptr()] for f, st in zip(flats, states)], dev)
    lib = L.load()
    if dtype == torch.float32:
        ws = _workspace(lib.oq_minmax_many_workspace_bytes(len(flats)), dev)
        L.check(lib.oq_minmax_collect_many_f32(_ptr(desc), len(flats), float(momentum), _ptr(ws), ws.numel(), _stream()))
    else:
        ws = _workspace(lib.oq_minmax_many_half_workspace_bytes(len(flats)), dev)
        L.check(lib.oq_minmax_collect_many_h16(_ptr(desc), len(flats), _HALF_WTYPE[dtype], float(momentum), _ptr(ws), ws.numel(), _stream()))


def absmax(x: torch.Tensor, per_row: bool = False) -> torch.Tensor:
    """smooth_quant.py:62-74: max |x| per last-axis channel ([..., C] -> [C]); per_row=True gives the
    per-row absmax of a 2-D matrix (weights [K, N] -> [K]).  fp32 out.  An fp16 / bf16 ``x`` is read as it is
    (`oq_absmax_h16`) and gives what ``absmax(x.float())`` gives, bit for bit."""
    half = isinstance(x, torch.Tensor) and x.dtype in _HALF_WTYPE
    _require_device(x, "x", None if half else torch.float32)
    x2 = x.reshape(-1, x.shape[-1])
    x2, ldx = _row_major(x2)
    r, c = x2.shape
    lib = L.load()
    out = torch.empty(r if per_row else c, dtype=torch.float32, device=x.device)
    xargs, kind = _twin(x2)
    ws = _workspace(getattr(lib, _TWIN_WORKSPACE["absmax"][kind])(r, c, int(per_row)), x.device)
    L.check(getattr(lib, "oq_absmax_" + kind)(*xargs, r, c, ldx, int(per_row), _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out


def abs_stats_accumulate_many(xs, abs_sums, absmaxes) -> None:
    """awq.py:47-50 / smooth_quant.py:62-69 as running statistics for a list of fp16 / bf16 tensors of ONE dtype, in ONE C call
    (`oq_abs_stats_cols_many_h16`, csrc/abs_stats_half.hip: two launches for the whole list): ``xs[i]`` [..., K_i] is read as it
    is, once, and folded into the fp32 ``abs_sums[i]`` [K_i] (+= sum over rows of |x|) and ``absmaxes[i]`` [K_i] (NaN-propagating
    maximum with max over rows of |x|), both updated in place.  The results are, bit for bit, those of the fp32 route on
    ``xs[i].float()``: `oq_abs_sum_cols_f32` accumulating, and ``torch.maximum(running, absmax(x.float()))``.
    The 48-byte items travel in one small host-to-device copy per call (none for a list of one)."""
    xs, abs_sums, absmaxes = list(xs), list(abs_sums), list(absmaxes)
    if not xs or not (len(xs) == len(abs_sums) == len(absmaxes)):
        raise ValueError("abs_stats_accumulate_many needs equally long, non-empty lists")
    dtype = xs[0].dtype if isinstance(xs[0], torch.Tensor) else None
    rows, keep = [], []
    for i, (x, sm, mx) in enumerate(zip(xs, abs_sums, absmaxes)):
        _require_device(x, "x")
        if x.dtype not in _HALF_WTYPE or dtype not in _HALF_WTYPE:
            raise TypeError(f"abs_stats_accumulate_many takes fp16 / bf16 tensors, got {x.dtype if dtype in _HALF_WTYPE else dtype}")
        if x.dtype != dtype:
            raise TypeError(f"abs_stats_accumulate_many takes tensors of one dtype per call, got {dtype} and {x.dtype}")
        if x.dim() < 1 or x.numel() == 0:
            raise ValueError(f"abs_stats_accumulate_many: x[{i}] is empty ({tuple(x.shape)})")
        x2, ldx = _row_major(x.reshape(-1, x.shape[-1]))
        t, k = x2.shape
        for name, out in (("abs_sums", sm), ("absmaxes", mx)):
            _require_device(out, f"{name}[{i}]", torch.float32)
            if out.shape != (k,) or not out.is_contiguous():
                raise ValueError(f"{name}[{i}] must be a contiguous [{k}] tensor")
        rows.append((x2.data_ptr(), t, k, ldx, sm.data_ptr(), mx.data_ptr()))
        keep.append(x2)
    lib = L.load()
    _host, hp, dev = _item_table(rows, keep[0].device if len(rows) > 1 else None)          # 48 bytes per item
    ws = _workspace(lib.oq_abs_stats_many_half_workspace_bytes(hp, len(rows)), keep[0].device)
    L.check(lib.oq_abs_stats_cols_many_h16(hp, _ptr(dev), len(rows), _HALF_WTYPE[dtype], _ptr(ws), ws.numel(), _stream()))


# ----------------------------------------------------------------------------- N2: AWQ / SmoothQuant searches
def _flat_inputs(x: torch.Tensor) -> torch.Tensor:
    _require_device(x, "inputs", torch.float32)
    return x.reshape(-1, x.shape[-1])


def _search_weight(w):
    """The weight of a search as the library takes it: fp32 for the `_f32` entry points, fp16 / bf16 AS IT IS for their `_h16`
    twins (csrc/awq.hip reads 2-byte elements and converts at the load).  No cast is made; any other dtype is refused by name."""
    if isinstance(w, torch.Tensor) and w.dtype in _HALF_WTYPE:
        _require_device(w, "w")
    else:
        _require_device(w, "w", torch.float32)
    return w


def _search_args(x, w, qtype, strategy, group_size):
    x2, ldx = _row_major(_flat_inputs(x))
    w = _search_weight(w)
    if w.dim() != 2 or w.shape[0] != x2.shape[1]:
        raise ValueError(f"weights must be [K, N] with K = {x2.shape[1]}, got {tuple(w.shape)}")
    w2, ldw = _row_major(w)
    if BITS[qtype] > 8:
        raise NotImplementedError("the AWQ searches take 4- and 8-bit types")
    gs = -1 if group_size is None else int(group_size)
    return x2, ldx, w2, ldw, gs


def _awq_search(entry, query, query_args, lead, w2, ldw, quant, n_losses, scales_k=None):
    """What the four AWQ searches share: the output buffers, the `_f32` / `_h16` twin of ``oq_<entry>``, its workspace (``query``
    of `_TWIN_WORKSPACE` on ``query_args``) aligned to 256 bytes, the call and the read-back.  ``lead``: the arguments in front of
    the weight (`_search_args`: X; `_stats_args`: the statistics); ``quant``: (qtype, strategy, gs, symmetric, reduce_range).
    A scale search passes its grid as ``n_losses`` and K as ``scales_k`` (the entry point then takes the grid and the candidate
    scales [n_losses, K]); a clip search passes its ten ratios and no ``scales_k``.
    Returns (scales on device | None, the winner's index, losses float64 on host)."""
    qtype, strategy, gs, symmetric, reduce_range = quant
    n = w2.shape[1]
    lib = L.load()
    dev = w2.device
    scales = None if scales_k is None else torch.empty((n_losses, scales_k), dtype=torch.float32, device=dev)
    losses = torch.empty(n_losses, dtype=torch.float32, device=dev)
    best = torch.zeros(1, dtype=torch.int32, device=dev)
    wargs, kind = _twin(w2)
    ws = _workspace(getattr(lib, _TWIN_WORKSPACE[query][kind])(*query_args) + 256, dev)
    off = (-ws.data_ptr()) % 256
    grid = () if scales is None else (int(n_losses), _ptr(scales))
    L.check(getattr(lib, f"oq_{entry}_{kind}")(*lead, *wargs, n, ldw, L.QTYPE_CODE[qtype], L.STRATEGY_CODE[strategy], gs, int(symmetric),
                                               int(reduce_range), *grid, _ptr(losses), _ptr(best), C.c_void_p(ws.data_ptr() + off),
                                               ws.numel() - off, _stream()))
    return scales, int(best.item()), losses.double().cpu().numpy()


def awq_scale_search(x: torch.Tensor, w: torch.Tensor, qtype: str, strategy: str, group_size, symmetric=False,
                     reduce_range=False, n_grid: int = 20):
    """pre_passes/awq.py:114-184 on the device, one C call (oq_awq_scale_search_f32): activation / weight statistics, the
    n_grid candidate scales, and per candidate RTN -> dequantize -> X (W - W^) on the matrix cores with the squared error
    reduced in the GEMM's epilogue.  Nothing leaves the GPU until the losses and the winning scale are read.
    ``x`` is fp32.  An fp16 / bf16 ``w`` is read as it is (oq_awq_scale_search_h16, no fp32 copy): every candidate scale, loss and
    the winner are those of the fp32 call on ``w.float()``, byte for byte.
    Returns (best_scale [K] on device, losses float64[n_grid] on host)."""
    x2, ldx, w2, ldw, gs = _search_args(x, w, qtype, strategy, group_size)
    t, k = x2.shape
    scales, best, lv = _awq_search("awq_scale_search", "awq", (t, k, w2.shape[1]), (_ptr(x2), t, k, ldx), w2, ldw,
                                   (qtype, strategy, gs, symmetric, reduce_range), n_grid, scales_k=k)
    return scales[best], lv


def awq_clip_search(x: torch.Tensor, w: torch.Tensor, qtype: str, strategy: str, group_size, symmetric=False,
                    reduce_range=False):
    """pre_passes/awq.py:207-259 (oq_awq_clip_search_f32): (best clip_ratio, losses[10]).  ``x`` is fp32; an fp16 / bf16 ``w`` is
    read as it is (oq_awq_clip_search_h16, no fp32 copy) and gives the losses and the ratio of ``w.float()``, byte for byte."""
    x2, ldx, w2, ldw, gs = _search_args(x, w, qtype, strategy, group_size)
    t, k = x2.shape
    _, best, lv = _awq_search("awq_clip_search", "awq", (t, k, w2.shape[1]), (_ptr(x2), t, k, ldx), w2, ldw,
                              (qtype, strategy, gs, symmetric, reduce_range), 10)
    return 1 - best / 100, lv


class SearchStatistics:
    """What the AWQ / SmoothQuant searches need of a calibration input, as running statistics over its batches (no batch is
    held): `gram` = (2 / rows) X^T X (the Hessian update rule of gptq.py:246-260 with n counting ROWS), `abs_sum[k]` = sum_t |x[t, k]|
    (awq.py:47-50 divides by the rows), `absmax[k]` = max_t |x[t, k]| (smooth_quant.py:62-69), `rows`.  `divide(scale)` is the
    reference's in-place rescale of the stored input (`node.meta["input"] /= scale`, awq.py:191 / smooth_quant.py:121) in these
    terms: the next consumer of the same value searches on what the previous one left.

    Batches may be fp32, fp16 or bf16: a half batch is read as it is (`abs_stats_accumulate_many`, `hessian_accumulate`) into the
    same fp32 statistics -- `abs_sum` and `absmax` with the bits the upcast batch gives, `gram` within the Hessian tolerance."""

    def __init__(self, k: int, device):
        self.gram = torch.zeros((k, k), dtype=torch.float32, device=device)
        self.abs_sum = torch.zeros(k, dtype=torch.float32, device=device)
        self.absmax = torch.zeros(k, dtype=torch.float32, device=device)
        self.rows = 0

    def add(self, x: torch.Tensor) -> None:
        """Fold one batch ``x`` [samples, ..., K] in.  An fp16 / bf16 ``x`` is read as it is: one `abs_stats_accumulate_many` call
        of one item (both |x| statistics in one pass, the bits of the fp32 route on ``x.float()``) and `hessian_accumulate` on the
        half tensor; no fp32 copy is made."""
        if isinstance(x, torch.Tensor) and x.dtype in _HALF_WTYPE:
            abs_stats_accumulate_many([x], [self.abs_sum], [self.absmax])
            self.rows = hessian_accumulate(x.reshape(-1, x.shape[-1]), self.gram, self.rows)
            return
        x2 = _flat_inputs(x if x.dtype == torch.float32 else x.to(torch.float32))
        x2, ldx = _row_major(x2)
        self._fold_abs(x2, ldx)
        self.rows = hessian_accumulate(x2, self.gram, self.rows)            # rows as samples: gram = (2 / rows) X^T X

    def _fold_abs(self, x2: torch.Tensor, ldx: int) -> None:
        """The |x| statistics of one fp32 batch ``x2`` [rows, K] with contiguous rows: the per-tensor kernels."""
        t, k = x2.shape
        lib = L.load()
        ws = _workspace(lib.oq_abs_sum_cols_workspace_bytes(k), x2.device)
        L.check(lib.oq_abs_sum_cols_f32(_ptr(x2), t, k, ldx, _ptr(self.abs_sum), 1, _ptr(ws), ws.numel(), _stream()))
        self.absmax = torch.maximum(self.absmax, absmax(x2))

    @staticmethod
    def add_many(stats: "list[SearchStatistics]", xs) -> None:
        """`add` for several values of one batch: the Gram updates in ONE grouped launch chain per element type
        (`hessian_accumulate_many`: a batch of a small model is dozens of small products, launch-bound one at a time), and the |x|
        statistics of the fp16 / bf16 values in one `abs_stats_accumulate_many` call per element type -- those are read as they
        are, no fp32 copy is made.  fp32 values take the per-tensor |x| kernels."""
        flat = []
        for x in xs:
            if isinstance(x, torch.Tensor) and x.dtype in _HALF_WTYPE:
                _require_device(x, "inputs")
                flat.append(_row_major(x.reshape(-1, x.shape[-1]))[0])
                continue
            x2 = _flat_inputs(x if x.dtype == torch.float32 else x.to(torch.float32))
            flat.append(_row_major(x2)[0])
        half: dict = {}                   # element type -> positions
        for i, (st, x2) in enumerate(zip(stats, flat)):
            if x2.dtype in _HALF_WTYPE:
                half.setdefault(x2.dtype, []).append(i)
            else:
                st._fold_abs(x2, x2.stride(0))
        for idx in half.values():
            abs_stats_accumulate_many([flat[i] for i in idx], [stats[i].abs_sum for i in idx], [stats[i].absmax for i in idx])
        if half or hessian_method() in ("auto", "f16x3"):                 # the method does not concern half items
            for st, n in zip(stats, hessian_accumulate_many(flat, [st.gram for st in stats], [st.rows for st in stats])):
                st.rows = n
        else:
            for st, x2 in zip(stats, flat):
                st.rows = hessian_accumulate(x2, st.gram, st.rows)

    def divide(self, scale: torch.Tensor) -> None:
        s = scale.to(self.gram.device, torch.float32).reshape(-1)
        self.abs_sum /= s
        self.absmax /= s
        self.gram /= s.reshape(-1, 1)
        self.gram /= s.reshape(1, -1)


def _stats_args(stats: "SearchStatistics", w, qtype, group_size):
    w = _search_weight(w)
    k = stats.gram.shape[0]
    if w.dim() != 2 or w.shape[0] != k:
        raise ValueError(f"weights must be [K, N] with K = {k}, got {tuple(w.shape)}")
    if stats.rows <= 0:
        raise ValueError("the statistics hold no calibration rows")
    if BITS[qtype] > 8:
        raise NotImplementedError("the AWQ searches take 4- and 8-bit types")
    w2, ldw = _row_major(w)
    return w2, ldw, k, w2.shape[1], (-1 if group_size is None else int(group_size))


def awq_scale_search_stats(stats: "SearchStatistics", w: torch.Tensor, qtype: str, strategy: str, group_size, symmetric=False,
                           reduce_range=False, n_grid: int = 20):
    """`awq_scale_search` from running statistics (oq_awq_scale_search_stats_f32): (best_scale [K] on device, losses[n_grid]).
    An fp16 / bf16 ``w`` is read as it is (oq_awq_scale_search_stats_h16, no fp32 copy); the arithmetic of the search is fp32 and the
    result that of ``w.float()``, byte for byte."""
    w2, ldw, k, n, gs = _stats_args(stats, w, qtype, group_size)
    scales, best, lv = _awq_search("awq_scale_search_stats", "awq_stats", (k, n), (_ptr(stats.abs_sum), _ptr(stats.gram), stats.rows, k), w2, ldw,
                                   (qtype, strategy, gs, symmetric, reduce_range), n_grid, scales_k=k)
    return scales[best], lv


def awq_clip_search_stats(stats: "SearchStatistics", w: torch.Tensor, qtype: str, strategy: str, group_size, symmetric=False,
                          reduce_range=False):
    """`awq_clip_search` from running statistics (oq_awq_clip_search_stats_f32): (best clip_ratio, losses[10]).
    An fp16 / bf16 ``w`` is read as it is (oq_awq_clip_search_stats_h16, no fp32 copy): the result of ``w.float()``, byte for byte."""
    w2, ldw, k, n, gs = _stats_args(stats, w, qtype, group_size)
    _, best, lv = _awq_search("awq_clip_search_stats", "awq_stats", (k, n), (_ptr(stats.gram), stats.rows, k), w2, ldw,
                              (qtype, strategy, gs, symmetric, reduce_range), 10)
    return 1 - best / 100, lv


def smooth_quant_scale_stats(stats: "SearchStatistics", w: torch.Tensor, alpha: float) -> torch.Tensor:
    """`smooth_quant_scale` from the running per-channel absmax: the kernel's column absmax of a one-row matrix is that row.
    An fp16 / bf16 ``w`` is read as it is (oq_smooth_quant_scale_h16)."""
    return smooth_quant_scale(stats.absmax.reshape(1, -1), w, alpha)


def smooth_quant_scale(x: torch.Tensor, w: torch.Tensor, alpha: float) -> torch.Tensor:
    """pre_passes/smooth_quant.py:62-74, :111-113 (oq_smooth_quant_scale_f32): the smoothing scale [K] on the device.  ``x`` is
    fp32; an fp16 / bf16 ``w`` is read as it is (oq_smooth_quant_scale_h16, no fp32 copy) and gives the scale of ``w.float()``, byte
    for byte."""
    x2, ldx = _row_major(_flat_inputs(x))
    w = _search_weight(w)
    t, k = x2.shape
    if w.dim() != 2 or w.shape[0] != k:           # the kernel reads K rows of W: a shorter W would be read out of bounds
        raise ValueError(f"weights must be [K, N] with K = {k}, got {tuple(w.shape)}")
    if w.device != x2.device:
        raise RuntimeError(f"inputs live on {x2.device} and weights on {w.device}")
    w2, ldw = _row_major(w)
    lib = L.load()
    out = torch.empty(k, dtype=torch.float32, device=w2.device)
    ws = _workspace(lib.oq_smooth_quant_workspace_bytes(k), w2.device)
    wargs, kind = _twin(w2)
    L.check(getattr(lib, "oq_smooth_quant_scale_" + kind)(_ptr(x2), t, k, ldx, *wargs, w2.shape[1], ldw, float(alpha), _ptr(out), _ptr(ws),
                                                          ws.numel(), _stream()))
    return out


# ----------------------------------------------------------------------------- N3
def pack_zero_points_u4(zp: torch.Tensor, n: int, blocks: int) -> torch.Tensor:
    """_common.py:96-121: [N*blocks] 4-bit zero points -> [N, ceil(blocks/2)] (pad nibble 0x8)."""
    _require_device(zp, "zp")
    z = zp.contiguous().reshape(-1).view(torch.uint8)
    out = torch.empty((n, (blocks + 1) // 2), dtype=torch.uint8, device=zp.device)
    L.check(L.load().oq_pack_zero_points_u4(_ptr(z), n, blocks, _ptr(out), _stream()))
    return out


def pack_matmul_nbits(q: torch.Tensor, group_size: int, bits: int) -> torch.Tensor:
    """_common.py:72-87: [K, N] 4- / 8-bit values (one per byte) -> the MatMulNBits blob [N, K/g, g*bits/8]."""
    _require_device(q, "q")
    if q.dim() != 2:
        raise ValueError("q must be [K, N]")
    k, n = q.shape
    v = q.contiguous().view(torch.uint8)
    out = torch.empty((n, k // group_size, group_size * bits // 8), dtype=torch.uint8, device=q.device)
    L.check(L.load().oq_pack_matmul_nbits(_ptr(v), k, n, int(group_size), int(bits), _ptr(out), _stream()))
    return out


def pack_nibbles(values: torch.Tensor) -> torch.Tensor:
    """_pack.py:8-22: flat 4-bit packing, element 2j in the low nibble."""
    _require_device(values, "values")
    v = values.contiguous().reshape(-1).view(torch.uint8)
    out = torch.empty((v.numel() + 1) // 2, dtype=torch.uint8, device=values.device)
    L.check(L.load().oq_pack_nibbles(_ptr(v), v.numel(), _ptr(out), _stream()))
    return out


# ----------------------------------------------------------------------------- N1: the calibration walk's large products
class MatmulOperand:
    """One operand of `matmul_pieces` split into fp16 pieces on the device (`oq_matmul_prepare_f32`).  A constant weight is
    prepared once and reused for every batch of the calibration walk."""

    __slots__ = ("pieces", "kd", "cols", "per_row")

    def __init__(self, pieces, kd, cols, per_row=False):
        self.pieces, self.kd, self.cols, self.per_row = pieces, kd, cols, per_row


def _aligned_bytes(nbytes: int, device) -> torch.Tensor:
    buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    off = (-buf.data_ptr()) % 256
    return buf[off:off + nbytes]


def matmul_prepare(t: torch.Tensor, contraction_is_fast_axis: bool, per_row: bool = False) -> MatmulOperand:
    """``t`` [cols, Kd] (activations: contraction on the fast axis) or [Kd, cols] (a weight) -> its fp16 pieces.  ``per_row``
    (activations only): one power-of-two scale per row instead of one for the operand."""
    _require_device(t, "operand", torch.float32)
    if t.dim() != 2:
        raise ValueError(f"matmul_prepare takes a matrix, got {tuple(t.shape)}")
    t2, ld = _row_major(t)
    cols, kd = (t2.shape[0], t2.shape[1]) if contraction_is_fast_axis else (t2.shape[1], t2.shape[0])
    lib = L.load()
    need = lib.oq_matmul_pieces_bytes(kd, cols)
    if need == 0:
        raise ValueError(f"matmul_prepare: an operand of {kd} x {cols} is too large for the piece kernels")
    pieces = _aligned_bytes(need, t2.device)
    L.check(lib.oq_matmul_prepare_f32(_ptr(t2), kd, cols, ld, 1 if contraction_is_fast_axis else 0, 1 if per_row else 0, _ptr(pieces), need,
                                      _stream()))
    return MatmulOperand(pieces, kd, cols, bool(per_row))


def matmul_pieces(x: torch.Tensor, w: MatmulOperand | torch.Tensor) -> torch.Tensor:
    """``x`` [..., Kd] fp32 times a weight [Kd, N] (a tensor, or its `matmul_prepare(w, False)` pieces) on the fp16 matrix
    cores with two-piece operands: 22 significand bits per operand, fp32 accumulate -- the arithmetic of the Hessian
    kernels.  Returns [..., N] fp32.  The weight is scaled as a whole and every ROW of ``x`` on its own by a power of two (any
    magnitude fp32 can hold): the 22 bits hold for elements within ~2^18 of their row's (the weight's) largest, whatever the other
    rows of the batch hold."""
    _require_device(x, "x", torch.float32)
    if not isinstance(w, MatmulOperand):
        w = matmul_prepare(w, False)
    x2 = x.reshape(-1, x.shape[-1])
    if x2.shape[1] != w.kd:
        raise ValueError(f"matmul_pieces: x has {x2.shape[1]} columns, the weight {w.kd} rows")
    a = matmul_prepare(x2, True, per_row=True)               # every row (token) keeps its own 22 bits, whatever its neighbours hold
    out = torch.empty((x2.shape[0], w.cols), dtype=torch.float32, device=x.device)
    L.check(L.load().oq_matmul_pieces_f32(_ptr(a.pieces), _ptr(w.pieces), x2.shape[0], w.cols, w.kd, 1.0, 0.0, _ptr(out), w.cols, 1, _stream()))
    return out.reshape(*x.shape[:-1], w.cols)


# ----------------------------------------------------------------------------- running a MatMulNBits node from its blob
_NBITS_TYPE = {torch.float32: L.OQ_NBITS_F32, torch.float16: L.OQ_NBITS_F16, torch.bfloat16: L.OQ_NBITS_BF16}


def matmul_nbits_unsupported(x_dtype, bits: int, block_size: int, zero_points=None, g_idx=None) -> str | None:
    """Why `matmul_nbits` has no kernel for such a node (include/oq_hip_nbits.h, "left out"), or None when it has one."""
    if x_dtype not in _NBITS_TYPE:
        return f"an input of {x_dtype} (fp32, fp16 and bf16 have a kernel)"
    if bits not in (4, 8):
        return f"bits = {bits} (4 and 8 have a kernel)"
    if block_size <= 0 or block_size % 32:
        return f"block_size = {block_size} is no multiple of 32 (two groups would share one 32-deep matrix instruction)"
    if zero_points is not None and zero_points.is_floating_point():
        return "float zero points (q - zp is no integer: no exact matrix-core operand)"
    if g_idx is not None:
        return "g_idx"
    return None


def matmul_nbits(x: torch.Tensor, blob: torch.Tensor, scales: torch.Tensor, zero_points: torch.Tensor | None = None, *, K: int, N: int,
                 bits: int, block_size: int, bias: torch.Tensor | None = None) -> torch.Tensor:
    """com.microsoft::MatMulNBits from the packed blob as stored (`oq_matmul_nbits`, csrc/matmul_nbits.hip): ``x`` [..., K] fp32,
    fp16 or bf16 times dequant(B)^T, B [N, ceil(K / block_size), block_size * bits / 8] uint8; ``scales`` [N, blocks] fp32 or of
    x's type; ``zero_points`` None (2^(bits - 1)) or uint8, for 4 bits packed two per byte; ``bias`` [N] of x's type.  Returns
    [..., N] of x's type.  (q - zp) meets x on the matrix cores as an exact integer operand, group sums are scaled in fp32: no
    [N, K] weight exists at any point.  Nothing synchronises with the host.

    NotImplementedError, naming the reason, for what the kernel leaves out: float zero points (HQQ), block sizes that are no
    multiple of 32 (16), bits other than 4 / 8."""
    return _nbits_call("matmul_nbits", x, blob, scales, zero_points, K, N, bits, block_size, bias, None, _nbits_tile_route)


# ----------------------------------------------------------------------------- the product of a QDQ function from its stored integers
_QDQ_WTYPE = {torch.uint8: L.OQ_UINT8, torch.int8: L.OQ_INT8}


def _qdq_granularity(count: int, k: int, n: int, g: int) -> tuple[int, int] | None:
    """(granularity code, group size handed to the library) read from the scale's element count: 1, N or N * K / g."""
    if g > 0 and k % g == 0 and count == n * (k // g):      # first: a per-column count is also that of one group of K
        return L.OQ_GROUP, g
    if g > 0:
        return None
    if count == 1:
        return L.OQ_TENSOR, 0
    if count == n:
        return L.OQ_CHANNEL, 0
    return None


def qdq_matmul_unsupported(x, w, scale, zero_point=None, *, group_size: int = 0, bias=None) -> str | None:
    """Why `qdq_matmul` has no kernel for such a product (include/oq_hip_qdq.h), or None when it has one.  Element types, shapes
    and the refusals of the entry point; where the tensors live is the caller's question."""
    if x.dtype not in _NBITS_TYPE:
        return f"an input of {x.dtype} (fp32, fp16 and bf16 have a kernel)"
    if w.dtype not in _QDQ_WTYPE or w.ndim != 2:
        return f"a weight of {w.dtype} and {w.ndim} axes (a uint8 / int8 [K, N] matrix has a kernel)"
    k, n, g = int(w.shape[0]), int(w.shape[1]), int(group_size)
    if x.ndim < 1 or x.shape[-1] != k:
        return f"an input whose last axis is not K = {k}"
    if g < 0 or (g and g % 32):
        return f"group_size = {g} is no multiple of 32 (two groups would share one 32-deep matrix instruction)"
    if g and k % g:
        return f"K = {k} is no multiple of group_size = {g}"
    if scale.dtype not in (torch.float32, x.dtype):
        return f"scales of {scale.dtype} (float32 and the input's type have a kernel)"
    if _qdq_granularity(scale.numel(), k, n, g) is None:
        return f"{scale.numel()} scales for a [{k}, {n}] weight and group_size = {g} (1, N or N * K / group_size)"
    if zero_point is not None and zero_point.dtype != w.dtype:
        return f"a zero point of {zero_point.dtype} for a weight of {w.dtype}"
    if zero_point is not None and zero_point.numel() != scale.numel():
        return f"{zero_point.numel()} zero points for {scale.numel()} scales"
    if bias is not None and (bias.dtype != x.dtype or bias.numel() != n):
        return f"a bias of {bias.numel()} x {bias.dtype} (N values of the input's type)"
    return None


def qdq_matmul(x: torch.Tensor, w: torch.Tensor, scale: torch.Tensor, zero_point: torch.Tensor | None = None, *, group_size: int = 0,
               bias: torch.Tensor | None = None) -> torch.Tensor:
    """The product of a `quant`-domain QDQ function from the integers it stores (`oq_qdq_matmul`, csrc/qdq_matmul.hip): ``x``
    [..., K] fp32, fp16 or bf16 times dequant(W), ``w`` [K, N] uint8 or int8 (rows may be strided); ``scale`` fp32 or of x's type
    with 1 (per tensor), N (per column) or N * K / group_size values (groups along K, entry n * (K / group_size) + k / group_size:
    the flat order of the grouped functions' blocked DequantizeLinear); ``zero_point`` None (0) or of w's type, indexed like the
    scale; ``bias`` [N] of x's type.  Returns [..., N] of x's type.  (q - zp) meets x on the matrix cores as an exact integer
    operand, group sums are scaled in fp32: no fp32 [K, N] weight exists at any point.  Nothing synchronises with the host.

    NotImplementedError, naming the reason, for what the kernel leaves out (`qdq_matmul_unsupported`)."""
    for t, name in ((x, "x"), (w, "w"), (scale, "scale")) + (((zero_point, "zero_point"),) if zero_point is not None else ()) + \
            (((bias, "bias"),) if bias is not None else ()):
        _require_device(t, name)
    why = qdq_matmul_unsupported(x, w, scale, zero_point, group_size=group_size, bias=bias)
    if why is not None:
        raise NotImplementedError(f"qdq_matmul: {why}")
    k, n = int(w.shape[0]), int(w.shape[1])
    granularity, g = _qdq_granularity(scale.numel(), k, n, int(group_size))
    w, ldw = _row_major(w)
    scale = scale.contiguous()
    zero_point = None if zero_point is None else zero_point.contiguous()
    bias = None if bias is None else bias.contiguous()
    rows = _rows_and_out(x.reshape(-1, k), n, x.dtype)
    if rows is None:
        return torch.zeros((*x.shape[:-1], n), dtype=x.dtype, device=x.device)
    x2, m, lda, out = rows
    lib = L.load()
    atype = _NBITS_TYPE[x.dtype]
    need = lib.oq_qdq_matmul_workspace_bytes(m, k, n, atype)
    ws = _workspace(need, x.device) if need else None
    L.check(lib.oq_qdq_matmul(_ptr(x2), atype, m, k, lda, _ptr(w), _QDQ_WTYPE[w.dtype], n, ldw, granularity, g, _ptr(scale), _NBITS_TYPE[scale.dtype],
                              _ptr(zero_point), _ptr(bias), _ptr(out), n, _ptr(ws), need, _stream()))
    return out.reshape(*x.shape[:-1], n)


DECODE_MAX_ROWS = 16      # include/oq_hip_nbits_decode.h: M of the decode route
_DECODE_WORKSPACE: dict = {}      # (M, K, N, block size, type code) -> oq_matmul_nbits_decode_workspace_bytes


def matmul_nbits_decode_unsupported(x_dtype, bits: int, block_size: int, zero_points=None, g_idx=None, rows: int | None = None) -> str | None:
    """Why `matmul_nbits_decode` has no kernel for such a node (include/oq_hip_nbits_decode.h, "left out"), or None when it has
    one.  ``rows``: the rows of the flattened input, where they are known."""
    if x_dtype not in _NBITS_TYPE:
        return f"an input of {x_dtype} (fp32, fp16 and bf16 have a kernel)"
    if rows is not None and rows > DECODE_MAX_ROWS:
        return f"{rows} rows (the decode route takes 1 ... {DECODE_MAX_ROWS}; matmul_nbits takes the rest)"
    if bits not in (4, 8):
        return f"bits = {bits} (4 and 8 have a kernel)"
    if block_size <= 0 or block_size % 16:
        return f"block_size = {block_size} is no multiple of 16 (a lane's unit of 16 k would straddle two groups)"
    if zero_points is not None and zero_points.is_floating_point() and zero_points.dtype not in (torch.float32, x_dtype):
        return f"zero points of {zero_points.dtype} (uint8, float32 and the input's type have a kernel)"
    if g_idx is not None:
        return "g_idx"
    return None


def _nbits_tile_route(lib, key, current):
    """`oq_matmul_nbits` with its workspace query, asked per call, on the current stream."""
    return lib.oq_matmul_nbits, lib.oq_matmul_nbits_workspace_bytes(*key), _stream()


def _nbits_decode_route(lib, key, current):
    """`oq_matmul_nbits_decode`: the call is made per token, so the workspace size is remembered per shape (a decode loop asks for
    the same few shapes thousands of times) and the stream handle taken raw."""
    need = _DECODE_WORKSPACE.get(key)
    if need is None:
        need = _DECODE_WORKSPACE[key] = lib.oq_matmul_nbits_decode_workspace_bytes(*key)
    return lib.oq_matmul_nbits_decode, need, C.c_void_p(_raw_stream(current))


def _nbits_float_zp_route(lib, key, current):
    """`oq_matmul_nbits_fzp` with its workspace query, asked per call, on the current stream."""
    return lib.oq_matmul_nbits_fzp, lib.oq_matmul_nbits_fzp_workspace_bytes(*key), _stream()


def _nbits_call(fn, x, blob, scales, zero_points, K, N, bits, block_size, bias, g_idx, route):
    """What `matmul_nbits`, `matmul_nbits_decode` and `matmul_nbits_float_zp` share: the checks, the operands as the C ABI wants
    them, the call.  ``route(lib, (M, K, N, block size, type code), current device)`` names the entry point, its workspace bytes
    and the stream.  The decode route also takes floating-point zero points (and says which kind they are: `zp_type`) and refuses
    by the rows; the float-zp route takes nothing else."""
    decode, float_zp = route is _nbits_decode_route, route is _nbits_float_zp_route
    current = None
    if decode:
        current = torch.cuda.current_device() if torch.cuda.is_available() else -1

        def require(t, name, dtype=None):      # `_require_device` with the current device asked for once: this call is made per token
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != current or (dtype is not None and t.dtype != dtype):
                _require_device(t, name, dtype)
    else:
        require = _require_device

    require(x, "x")
    K, N, bits, g = int(K), int(N), int(bits), int(block_size)
    why = None if decode else matmul_nbits_float_zp_unsupported(x.dtype, bits, g, zero_points, g_idx) if float_zp else \
        matmul_nbits_unsupported(x.dtype, bits, g, zero_points)
    if why is None and x.shape[-1] != K:
        raise ValueError(f"{fn}: x has {x.shape[-1]} columns, the node K = {K}")
    x2 = None
    if decode:      # its refusals name the rows, which the columns have to be right for
        x2 = x.reshape(-1, K)
        why = matmul_nbits_decode_unsupported(x.dtype, bits, g, zero_points, g_idx, rows=x2.shape[0])
    if why is not None:
        raise NotImplementedError(f"{fn}: {why}")
    blocks = (K + g - 1) // g
    require(blob, "blob", torch.uint8)
    if blob.numel() != N * blocks * (g * bits // 8):
        raise ValueError(f"{fn}: a blob of {N} x {blocks} x {g * bits // 8} bytes is expected, got {tuple(blob.shape)}")
    blob = blob.contiguous()
    require(scales, "scales")
    if scales.dtype not in (torch.float32, x.dtype) or scales.numel() != N * blocks:
        raise ValueError(f"{fn}: scales must be {N * blocks} values of float32 or {x.dtype}, got {scales.numel()} of {scales.dtype}")
    scales = scales.contiguous()
    zp_type = (L.OQ_NBITS_ZP_PACKED_U8,) if decode else ()      # an argument of the decode entry point alone
    if zero_points is not None:
        expect = N * ((blocks + 1) // 2) if bits == 4 else N * blocks      # uint8, for 4 bits packed
        if float_zp:      # floating point, of float32 or x's type: `matmul_nbits_float_zp_unsupported` has seen to it
            require(zero_points, "zero_points")
            expect, zp_type = N * blocks, (_NBITS_TYPE[zero_points.dtype],)
            if zero_points.numel() != expect:
                raise ValueError(f"{fn}: {expect} zero points ({zero_points.dtype}) are expected, got {zero_points.numel()}")
        elif not decode:
            require(zero_points, "zero_points", torch.uint8)
            if zero_points.numel() != expect:
                raise ValueError(f"{fn}: {expect} zero-point bytes are expected, got {zero_points.numel()}")
        else:
            require(zero_points, "zero_points")
            if zero_points.is_floating_point():
                expect, zp_type = N * blocks, (_NBITS_TYPE[zero_points.dtype],)
            elif zero_points.dtype != torch.uint8:
                raise ValueError(f"{fn}: zero points must be uint8 or floating point, got {zero_points.dtype}")
            if zero_points.numel() != expect:
                raise ValueError(f"{fn}: {expect} zero points ({zero_points.dtype}) are expected, got {zero_points.numel()}")
        zero_points = zero_points.contiguous()
    if bias is not None:
        require(bias, "bias", x.dtype)
        if bias.numel() != N:
            raise ValueError(f"{fn}: bias must hold {N} values, got {bias.numel()}")
        bias = bias.contiguous()
    rows = _rows_and_out(x.reshape(-1, K) if x2 is None else x2, N, x.dtype)
    if rows is None:
        return torch.zeros((*x.shape[:-1], N), dtype=x.dtype, device=x.device)
    x2, m, lda, out = rows
    atype = _NBITS_TYPE[x.dtype]
    entry, need, stream = route(L.load(), (m, K, N, g, atype), current)
    ws = _workspace(need, x.device) if need else None
    L.check(entry(_ptr(x2), atype, m, K, lda, _ptr(blob), bits, N, g, _ptr(scales), _NBITS_TYPE[scales.dtype], _ptr(zero_points), *zp_type,
                  _ptr(bias), 0, _ptr(out), N, _ptr(ws), need, stream))
    return out.reshape(*x.shape[:-1], N)


def matmul_nbits_decode(x: torch.Tensor, blob: torch.Tensor, scales: torch.Tensor, zero_points: torch.Tensor | None = None, *, K: int,
                        N: int, bits: int, block_size: int, bias: torch.Tensor | None = None, g_idx: torch.Tensor | None = None) -> torch.Tensor:
    """The decode route of com.microsoft::MatMulNBits (`oq_matmul_nbits_decode`, csrc/matmul_nbits_decode.hip): the operands and
    shape conventions of `matmul_nbits`, for an ``x`` whose ``reshape(-1, K)`` has 1 ... 16 rows.  The blob is streamed once
    from global memory into registers and dequantized there (fp32 on the vector ALU; from 5 rows on, where a group is a whole
    number of wave spans, on the matrix cores), so ``zero_points`` may also be floating point [N, blocks] (float32 or x's type:
    HQQ files) and ``block_size`` any multiple of 16.  Deterministic; nothing synchronises with the host.

    NotImplementedError, naming the reason, for what the kernel leaves out: more than 16 rows, block sizes that are no multiple
    of 16, bits other than 4 / 8, and a node that carries ``g_idx``."""
    return _nbits_call("matmul_nbits_decode", x, blob, scales, zero_points, K, N, bits, block_size, bias, g_idx, _nbits_decode_route)


def matmul_nbits_float_zp_unsupported(x_dtype, bits: int, block_size: int, zero_points, g_idx=None) -> str | None:
    """Why `matmul_nbits_float_zp` has no kernel for such a node (include/oq_hip_nbits_fzp.h, "left out"), or None when it has
    one."""
    if x_dtype not in _NBITS_TYPE:
        return f"an input of {x_dtype} (fp32, fp16 and bf16 have a kernel)"
    if bits not in (4, 8):
        return f"bits = {bits} (4 and 8 have a kernel)"
    if block_size <= 0 or block_size % 32:
        return f"block_size = {block_size} is no multiple of 32 (two groups would share one 32-deep matrix instruction)"
    if zero_points is None or not zero_points.is_floating_point():
        return "integer zero points (matmul_nbits is their route)"
    if zero_points.dtype not in (torch.float32, x_dtype):
        return f"zero points of {zero_points.dtype} (float32 and the input's type have a kernel)"
    if g_idx is not None:
        return "g_idx"
    return None


def matmul_nbits_float_zp(x: torch.Tensor, blob: torch.Tensor, scales: torch.Tensor, zero_points: torch.Tensor, *, K: int, N: int,
                          bits: int, block_size: int, bias: torch.Tensor | None = None) -> torch.Tensor:
    """com.microsoft::MatMulNBits with floating-point zero points (HQQ files), any number of rows, from the packed blob as stored
    (`oq_matmul_nbits_fzp`, csrc/matmul_nbits_fzp.hip): the operands and shape conventions of `matmul_nbits`, with
    ``zero_points`` [N, blocks] of float32 or x's type.  Every zero point is split into zi = clamp(rint(zp), 0, 2^bits - 1) and
    f = zp - zi: (q - zi) meets x on the matrix cores as an exact integer operand, and a group's sum loses f times the sum of
    x's row over the group, taken by the same instructions.  No [N, K] weight exists at any point; nothing synchronises with
    the host.

    NotImplementedError, naming the reason, for what the kernel leaves out: integer zero points (`matmul_nbits` is their
    route), block sizes that are no multiple of 32, bits other than 4 / 8."""
    return _nbits_call("matmul_nbits_float_zp", x, blob, scales, zero_points, K, N, bits, block_size, bias, None, _nbits_float_zp_route)


# ----------------------------------------------------------------------------- QLinearMatMul / QGemm / MatMulInteger on the int8 matrix cores
_QL_TYPE = {torch.uint8: L.OQ_QL_U8, torch.int8: L.OQ_QL_I8}
_QL_OUT = {torch.int32: L.OQ_QL_OUT_I32, torch.float32: L.OQ_QL_OUT_F32, torch.uint8: L.OQ_QL_OUT_U8, torch.int8: L.OQ_QL_OUT_I8}


def qlinear_matmul_unsupported(a, a_scale, a_zero_point, b, b_scale, b_zero_point, y_scale=None, y_zero_point=None, *, bias=None,
                               trans_b: bool = False, alpha: float = 1.0, trans_a: bool = False) -> str | None:
    """Why `qlinear_matmul` has no kernel for such operands (include/oq_hip_qlinear.h, "left out"), or None when it has one.
    The scales may be None (`matmul_integer`)."""
    if trans_a:
        return "transA"
    if alpha != 1.0:
        return f"alpha = {alpha} (only alpha = 1 has a kernel)"
    if a.dtype not in _QL_TYPE or b.dtype not in _QL_TYPE:
        return f"operands of {a.dtype} and {b.dtype} (uint8 and int8 have a kernel)"
    if b.ndim != 2:
        return f"a {b.ndim}-D b (a 2-D weight has a kernel)"
    if a.ndim < 1 or a.shape[-1] != b.shape[1 if trans_b else 0]:
        return f"shapes {tuple(a.shape)} and {tuple(b.shape)} do not meet (trans_b = {bool(trans_b)})"
    n = b.shape[0 if trans_b else 1]
    for name, s in (("a_scale", a_scale), ("b_scale", b_scale), ("y_scale", y_scale)):
        if s is not None and s.dtype != torch.float32:
            return f"{name} of {s.dtype} (scales that are not fp32 have no kernel)"
    if (a_scale is not None and a_scale.numel() != 1) or (a_zero_point is not None and a_zero_point.numel() != 1):
        return "a per-row a_scale / a_zero_point (activation parameters per tensor have a kernel)"
    if b_scale is not None and b_scale.numel() not in (1, n):
        return f"b_scale of {b_scale.numel()} values (1 or N = {n})"
    if b_zero_point is not None and b_zero_point.numel() not in (1, n):
        return f"b_zero_point of {b_zero_point.numel()} values (1 or N = {n})"
    if b_scale is not None and b_zero_point is not None and b_scale.numel() != b_zero_point.numel() and 1 not in (b_scale.numel(), b_zero_point.numel()):
        return "b_scale and b_zero_point of different lengths"
    if (y_scale is not None and y_scale.numel() != 1) or (y_zero_point is not None and y_zero_point.numel() != 1):
        return "a per-row or per-column y_scale / y_zero_point"
    if a_zero_point is not None and a_zero_point.dtype != a.dtype:
        return f"a_zero_point of {a_zero_point.dtype} for an a of {a.dtype}"
    if b_zero_point is not None and b_zero_point.dtype != b.dtype:
        return f"b_zero_point of {b_zero_point.dtype} for a b of {b.dtype}"
    if y_zero_point is not None and y_zero_point.dtype not in _QL_TYPE:
        return f"y_zero_point of {y_zero_point.dtype}"
    if bias is not None and (bias.dtype != torch.int32 or bias.numel() != n):
        return f"a bias of {bias.numel()} values of {bias.dtype} (int32 [N = {n}])"
    return None


def _tile_route(lib, m, k, n, trans_b, current):
    """`oq_qlinear_matmul` with its workspace query, asked per call, on the current stream."""
    return lib.oq_qlinear_matmul, lib.oq_qlinear_matmul_workspace_bytes(m, k, n), _stream()


_QL_DECODE_WORKSPACE: dict = {}      # (M, K, N, layout code) -> oq_qlinear_matmul_decode_workspace_bytes


def _decode_route(lib, m, k, n, trans_b, current):
    """`oq_qlinear_matmul_decode`: the call is made per token, so the workspace size is remembered per shape and the stream handle
    taken raw (docs/LAB_NOTES_r26.md, section 4)."""
    key = (m, k, n, L.OQ_QL_NK if trans_b else L.OQ_QL_KN)
    need = _QL_DECODE_WORKSPACE.get(key)
    if need is None:
        need = _QL_DECODE_WORKSPACE[key] = lib.oq_qlinear_matmul_decode_workspace_bytes(*key)
    return lib.oq_qlinear_matmul_decode, need, C.c_void_p(_raw_stream(current))


def _qlinear_call(fn, a, a_scale, a_zero_point, b, b_scale, b_zero_point, y_scale, y_zero_point, bias, trans_b, alpha, trans_a, out_dtype,
                  route=_tile_route, unsupported=None, codes=None):
    """What `qlinear_matmul` / `matmul_integer`, their decode twins and `qlinear_function` / `qlinear_function_decode` share: the
    checks, the operands as the C ABI wants them, the call.  ``route(lib, m, k, n, trans_b, current device)`` names the entry
    point, its workspace bytes and the stream; ``unsupported`` the refusals of that entry point (by default
    `qlinear_matmul_unsupported`); ``codes``: (a_type, the code in the place of `out`) where they are not those of ``a``'s and the
    result's element types (the function entry points: fp32 on both sides)."""
    current = None
    if route is _tile_route:
        require = _require_device
    else:
        current = torch.cuda.current_device() if torch.cuda.is_available() else -1

        def require(t, name):      # `_require_device` with the current device asked for once
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != current:
                _require_device(t, name)

    require(a, "a")
    require(b, "b")
    params = dict(a_scale=a_scale, a_zero_point=a_zero_point, b_scale=b_scale, b_zero_point=b_zero_point, y_scale=y_scale,
                  y_zero_point=y_zero_point, bias=bias)
    for name, t in params.items():
        if t is not None:
            require(t, name)
    why = (unsupported or qlinear_matmul_unsupported)(a, a_scale, a_zero_point, b, b_scale, b_zero_point, y_scale, y_zero_point, bias=bias,
                                                      trans_b=trans_b, alpha=alpha, trans_a=trans_a)
    if why is not None:
        raise NotImplementedError(f"{fn}: {why}")
    k = a.shape[-1]
    n = b.shape[0 if trans_b else 1]
    a2 = a.reshape(-1, k)
    if a2.shape[0] == 0:
        return torch.zeros((*a.shape[:-1], n), dtype=out_dtype, device=a.device)
    a2, lda = _row_major(a2)
    b, ldb = _row_major(b)
    m = a2.shape[0]
    # one zero point for every column next to per-column scales (or the reverse): the library takes one flag for both
    per_column = any(t is not None and t.numel() == n and n > 1 for t in (b_scale, b_zero_point))
    if per_column:
        if b_scale is not None and b_scale.numel() == 1:
            b_scale = b_scale.reshape(1).expand(n)
        if b_zero_point is not None and b_zero_point.numel() == 1:
            b_zero_point = b_zero_point.reshape(1).expand(n)
    a_scale, a_zero_point, b_scale, b_zero_point, y_scale, y_zero_point, bias = (
        None if t is None else t.contiguous() for t in (a_scale, a_zero_point, b_scale, b_zero_point, y_scale, y_zero_point, bias))
    out = torch.empty((m, n), dtype=out_dtype, device=a.device)
    lib = L.load()
    entry, need, stream = route(lib, m, k, n, trans_b, current)
    ws = _workspace(need, a.device) if need or route is _tile_route else None
    a_code, out_code = codes if codes is not None else (_QL_TYPE[a.dtype], _QL_OUT[out_dtype])
    L.check(entry(_ptr(a2), a_code, m, k, lda, _ptr(a_scale), _ptr(a_zero_point), _ptr(b), _QL_TYPE[b.dtype],
                  L.OQ_QL_NK if trans_b else L.OQ_QL_KN, n, ldb, _ptr(b_scale), _ptr(b_zero_point), int(per_column), _ptr(bias),
                  _ptr(y_scale), _ptr(y_zero_point), 0, out_code, _ptr(out), n, _ptr(ws), need, stream))
    return out.reshape(*a.shape[:-1], n)


def qlinear_matmul(a: torch.Tensor, a_scale: torch.Tensor, a_zero_point: torch.Tensor | None, b: torch.Tensor, b_scale: torch.Tensor,
                   b_zero_point: torch.Tensor | None, y_scale: torch.Tensor | None = None, y_zero_point: torch.Tensor | None = None, *,
                   bias: torch.Tensor | None = None, trans_b: bool = False, alpha: float = 1.0, trans_a: bool = False) -> torch.Tensor:
    """QLinearMatMul / com.microsoft::QGemm on the int8 matrix cores (`oq_qlinear_matmul`, csrc/qlinear_gemm.hip): ``a`` [..., K]
    uint8 / int8 times ``b`` [K, N] (``trans_b``: [N, K]) uint8 / int8, each minus its zero point, summed exactly in int32, plus
    ``bias`` (int32 [N], at scale a_scale * b_scale).  Every parameter is a tensor on the device: ``a_scale`` / ``a_zero_point``
    per tensor, ``b_scale`` / ``b_zero_point`` per tensor or [N]; a zero point of None is 0.  With ``y_scale`` the result is
    rint(fp32(acc) * fl(a_scale * b_scale) / y_scale) + y_zero_point, saturated, in ``y_zero_point``'s type (uint8 without one);
    without ``y_scale`` it is the fp32 value fp32(acc) * fl(a_scale * b_scale).  No operand is ever dequantized in memory, and
    nothing synchronises with the host.

    NotImplementedError, naming the reason, for what the kernel leaves out: per-row activation parameters, a ``b`` that is not
    2-D, scales that are not fp32, ``alpha`` != 1, ``trans_a``."""
    if a_scale is None or b_scale is None:
        raise ValueError("qlinear_matmul: a_scale and b_scale are required (matmul_integer runs without scales)")
    out_dtype = torch.float32 if y_scale is None else (torch.uint8 if y_zero_point is None else y_zero_point.dtype)
    return _qlinear_call("qlinear_matmul", a, a_scale, a_zero_point, b, b_scale, b_zero_point, y_scale, None if y_scale is None else y_zero_point,
                         bias, trans_b, alpha, trans_a, out_dtype)


def matmul_integer(a: torch.Tensor, b: torch.Tensor, a_zero_point: torch.Tensor | None = None, b_zero_point: torch.Tensor | None = None, *,
                   trans_b: bool = False) -> torch.Tensor:
    """MatMulInteger: sum_k (a - a_zero_point) * (b - b_zero_point) as int32, exact (two's-complement wrap), on the int8 matrix
    cores; operands and zero points as in `qlinear_matmul`."""
    return _qlinear_call("matmul_integer", a, None, a_zero_point, b, None, b_zero_point, None, None, None, trans_b, 1.0, False, torch.int32)


QL_DECODE_MAX_ROWS = 16      # include/oq_hip_qlinear_decode.h: M of the decode route


def qlinear_matmul_decode_unsupported(a, a_scale, a_zero_point, b, b_scale, b_zero_point, y_scale=None, y_zero_point=None, *, bias=None,
                                      trans_b: bool = False, alpha: float = 1.0, trans_a: bool = False, rows: int | None = None) -> str | None:
    """Why `qlinear_matmul_decode` has no kernel for such operands (include/oq_hip_qlinear_decode.h, "left out"), or None when it has
    one: what `qlinear_matmul_unsupported` names, and more than 16 rows.  ``rows``: the rows of the flattened ``a`` (asked from
    ``a`` itself where it is None)."""
    why = qlinear_matmul_unsupported(a, a_scale, a_zero_point, b, b_scale, b_zero_point, y_scale, y_zero_point, bias=bias, trans_b=trans_b,
                                     alpha=alpha, trans_a=trans_a)
    if why is not None:
        return why
    if rows is None:
        rows = a.numel() // a.shape[-1] if a.shape[-1] else 0
    if rows > QL_DECODE_MAX_ROWS:
        return f"{rows} rows (the decode route takes 1 ... {QL_DECODE_MAX_ROWS}; qlinear_matmul takes the rest)"
    return None


def qlinear_matmul_decode(a: torch.Tensor, a_scale: torch.Tensor, a_zero_point: torch.Tensor | None, b: torch.Tensor, b_scale: torch.Tensor,
                          b_zero_point: torch.Tensor | None, y_scale: torch.Tensor | None = None, y_zero_point: torch.Tensor | None = None, *,
                          bias: torch.Tensor | None = None, trans_b: bool = False, alpha: float = 1.0, trans_a: bool = False) -> torch.Tensor:
    """The decode route of QLinearMatMul / com.microsoft::QGemm (`oq_qlinear_matmul_decode`, csrc/qlinear_decode.hip): the operands
    and conventions of `qlinear_matmul`, for an ``a`` whose ``reshape(-1, K)`` has 1 ... 16 rows.  ``b`` is streamed once from
    global memory into registers (signed dot4 products; its column sums come from the same registers), the accumulator and the
    epilogue are those of `qlinear_matmul`, so the result has the same bytes.  Deterministic; nothing synchronises with the host.

    NotImplementedError, naming the reason, for what the kernel leaves out: more than 16 rows, and what `qlinear_matmul` refuses."""
    if a_scale is None or b_scale is None:
        raise ValueError("qlinear_matmul_decode: a_scale and b_scale are required (matmul_integer_decode runs without scales)")
    out_dtype = torch.float32 if y_scale is None else (torch.uint8 if y_zero_point is None else y_zero_point.dtype)
    return _qlinear_call("qlinear_matmul_decode", a, a_scale, a_zero_point, b, b_scale, b_zero_point, y_scale,
                         None if y_scale is None else y_zero_point, bias, trans_b, alpha, trans_a, out_dtype, route=_decode_route,
                         unsupported=qlinear_matmul_decode_unsupported)


def matmul_integer_decode(a: torch.Tensor, b: torch.Tensor, a_zero_point: torch.Tensor | None = None, b_zero_point: torch.Tensor | None = None, *,
                          trans_b: bool = False) -> torch.Tensor:
    """MatMulInteger on the decode route: `matmul_integer` for an ``a`` of 1 ... 16 rows, the same int32 values."""
    return _qlinear_call("matmul_integer_decode", a, None, a_zero_point, b, None, b_zero_point, None, None, None, trans_b, 1.0, False, torch.int32,
                         route=_decode_route, unsupported=qlinear_matmul_decode_unsupported)


def qlinear_function_unsupported(x, x_scale, x_zero_point, w, w_scale, w_zero_point, out_scale, out_zero_point, *, bias=None,
                                 trans_b: bool = False) -> str | None:
    """Why `qlinear_function` has no kernel for such operands (include/oq_hip_qlinear_function.h, "left out"), or None when it has
    one: an ``x`` that is not fp32, a missing scale, and what `qlinear_matmul_unsupported` names for the product inside."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        return f"an x of {getattr(x, 'dtype', type(x).__name__)} (fp32 has a kernel)"
    if x_scale is None or w_scale is None or out_scale is None:
        return "a missing x_scale, w_scale or out_scale (the function has all three)"
    a_dtype = torch.uint8 if x_zero_point is None else x_zero_point.dtype
    if a_dtype not in _QL_TYPE:
        return f"x_zero_point of {a_dtype} (uint8 and int8 have a kernel)"
    quantized = torch.empty(x.shape, dtype=a_dtype, device="meta")      # what QuantizeLinear would hand to the product: shape and type
    return qlinear_matmul_unsupported(quantized, x_scale, x_zero_point, w, w_scale, w_zero_point, out_scale, out_zero_point, bias=bias,
                                      trans_b=trans_b)


def qlinear_function_decode_unsupported(x, x_scale, x_zero_point, w, w_scale, w_zero_point, out_scale, out_zero_point, *, bias=None,
                                        trans_b: bool = False, rows: int | None = None) -> str | None:
    """Why `qlinear_function_decode` has no kernel for such operands, or None when it has one: what `qlinear_function_unsupported`
    names, and more than 16 rows.  ``rows``: the rows of the flattened ``x`` (asked from ``x`` itself where it is None)."""
    why = qlinear_function_unsupported(x, x_scale, x_zero_point, w, w_scale, w_zero_point, out_scale, out_zero_point, bias=bias, trans_b=trans_b)
    if why is not None:
        return why
    if rows is None:
        rows = x.numel() // x.shape[-1] if x.shape[-1] else 0
    if rows > QL_DECODE_MAX_ROWS:
        return f"{rows} rows (the decode route takes 1 ... {QL_DECODE_MAX_ROWS}; qlinear_function takes the rest)"
    return None


def _function_route(lib, m, k, n, trans_b, current):
    """`oq_qlinear_function` with its workspace query, asked per call, on the current stream."""
    return lib.oq_qlinear_function, lib.oq_qlinear_function_workspace_bytes(m, k, n), _stream()


_QL_FUNCTION_DECODE_WORKSPACE: dict = {}      # (M, K, N, layout code) -> oq_qlinear_function_decode_workspace_bytes


def _function_decode_route(lib, m, k, n, trans_b, current):
    """`oq_qlinear_function_decode`, per token: the workspace size remembered per shape, the stream handle taken raw (`_decode_route`)."""
    key = (m, k, n, L.OQ_QL_NK if trans_b else L.OQ_QL_KN)
    need = _QL_FUNCTION_DECODE_WORKSPACE.get(key)
    if need is None:
        need = _QL_FUNCTION_DECODE_WORKSPACE[key] = lib.oq_qlinear_function_decode_workspace_bytes(*key)
    return lib.oq_qlinear_function_decode, need, C.c_void_p(_raw_stream(current))


def _qlinear_function_call(fn, x, x_scale, x_zero_point, w, w_scale, w_zero_point, out_scale, out_zero_point, bias, trans_b, route, unsupported):
    def refusal(a, *rest, alpha, trans_a, **kw):      # `_qlinear_call` also names alpha and transA, which a function call has not
        return unsupported(a, *rest, **kw)

    codes = (_QL_TYPE.get(torch.uint8 if x_zero_point is None else x_zero_point.dtype, -1),
             _QL_TYPE.get(torch.uint8 if out_zero_point is None else out_zero_point.dtype, -1))      # y_type: an oq_ql_type
    return _qlinear_call(fn, x, x_scale, x_zero_point, w, w_scale, w_zero_point, out_scale, out_zero_point, bias, trans_b, 1.0, False,
                         torch.float32, route=route, unsupported=refusal, codes=codes)


def qlinear_function(x: torch.Tensor, x_scale: torch.Tensor, x_zero_point: torch.Tensor | None, w: torch.Tensor, w_scale: torch.Tensor,
                     w_zero_point: torch.Tensor | None, out_scale: torch.Tensor, out_zero_point: torch.Tensor | None, *,
                     bias: torch.Tensor | None = None, trans_b: bool = False) -> torch.Tensor:
    """One call of a `quant`-domain function QLinearMatMul / QLinearGemm of a ``format="qlinear"`` file (`oq_qlinear_function`,
    csrc/qlinear_function.hip): QuantizeLinear(x, x_scale, x_zero_point) -> QLinearMatMul / QGemm against ``w`` [K, N] (``trans_b``:
    [N, K]) -> DequantizeLinear(., out_scale, out_zero_point), fp32 ``x`` [..., K] in and fp32 [..., N] out, with the bytes of the
    three nodes run one after the other.  ``x`` is quantized to ``x_zero_point``'s type (uint8 without one) once, into the call's
    workspace; the product is exact in int32 (``bias``: int32 [N] at scale x_scale * w_scale); the result is quantized to
    ``out_zero_point``'s type (uint8 without one) and dequantized in the kernel's epilogue.  Every parameter is a tensor on the
    device, per tensor (``w_scale`` / ``w_zero_point``: per tensor or [N]).  A NaN in ``x`` quantizes to the bottom of the type.
    Deterministic; nothing synchronises with the host.

    NotImplementedError, naming the reason, for what the kernel leaves out: an ``x`` that is not fp32, and what `qlinear_matmul`
    refuses for the product."""
    return _qlinear_function_call("qlinear_function", x, x_scale, x_zero_point, w, w_scale, w_zero_point, out_scale, out_zero_point, bias, trans_b,
                                  _function_route, qlinear_function_unsupported)


def qlinear_function_decode(x: torch.Tensor, x_scale: torch.Tensor, x_zero_point: torch.Tensor | None, w: torch.Tensor, w_scale: torch.Tensor,
                            w_zero_point: torch.Tensor | None, out_scale: torch.Tensor, out_zero_point: torch.Tensor | None, *,
                            bias: torch.Tensor | None = None, trans_b: bool = False) -> torch.Tensor:
    """The decode route of `qlinear_function` (`oq_qlinear_function_decode`): the same operands, for an ``x`` whose ``reshape(-1, K)``
    has 1 ... 16 rows.  The kernels of `qlinear_matmul_decode` -- ``w`` streamed once -- quantize their slice of ``x`` on the way
    into LDS and dequantize in the epilogue: at most two launches, and the bytes of `qlinear_function`.

    NotImplementedError, naming the reason: more than 16 rows, and what `qlinear_function` refuses."""
    return _qlinear_function_call("qlinear_function_decode", x, x_scale, x_zero_point, w, w_scale, w_zero_point, out_scale, out_zero_point, bias,
                                  trans_b, _function_decode_route, qlinear_function_decode_unsupported)


# ----------------------------------------------------------------------------- a QDQ function with quantized activations in one call
QDQ_FUNCTION_MAX_K = 33025      # include/oq_hip_qdq_function.h, `bounds`: 255 * 255 * K stays an int32
_QDQ_MODE = {"static": L.OQ_QDQ_STATIC, "dynamic": L.OQ_QDQ_DYNAMIC, None: L.OQ_QDQ_NONE}


def qdq_function_unsupported(x, w, w_scale, w_zero_point=None, *, x_mode, x_scale=None, x_zero_point=None, out_mode=None, out_scale=None,
                             out_zero_point=None, bias=None) -> str | None:
    """Why `qdq_function` has no kernel for such a call (include/oq_hip_qdq_function.h, "left out"), or None when it has one.
    Element types, shapes and the refusals of the entry point; where the tensors live is the caller's question."""
    if x_mode not in ("static", "dynamic"):
        return f"x_mode = {x_mode!r} ('static' and 'dynamic' have a kernel; a function without an input Q -> DQ keeps qdq_matmul)"
    if out_mode not in (None, "static", "dynamic"):
        return f"out_mode = {out_mode!r} (None, 'static' and 'dynamic' have a kernel)"
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        return f"an x of {getattr(x, 'dtype', type(x).__name__)} (fp32 has a kernel)"
    if w.dtype not in _QDQ_WTYPE or w.ndim != 2:
        return f"a weight of {w.dtype} and {w.ndim} axes (a uint8 / int8 [K, N] matrix has a kernel)"
    k, n = int(w.shape[0]), int(w.shape[1])
    if x.ndim < 1 or x.shape[-1] != k:
        return f"an input whose last axis is not K = {k}"
    if k > QDQ_FUNCTION_MAX_K:
        return f"K = {k} (beyond {QDQ_FUNCTION_MAX_K} an int32 sum of 8-bit products could wrap)"
    if w_scale is None:
        return "a missing w_scale"
    if w_scale.dtype != torch.float32 or w_scale.numel() not in (1, n):
        return f"a w_scale of {w_scale.numel()} x {w_scale.dtype} (1 or N fp32 values: a grouped W keeps qdq_matmul)"
    if w_zero_point is not None and (w_zero_point.dtype != w.dtype or w_zero_point.numel() not in (1, n)):
        return f"a w_zero_point of {w_zero_point.numel()} x {w_zero_point.dtype} for a weight of {w.dtype}"
    for mode, scale, zp, name in ((x_mode, x_scale, x_zero_point, "x"), (out_mode, out_scale, out_zero_point, "out")):
        if mode != "static":
            continue
        if scale is None or scale.dtype != torch.float32 or scale.numel() != 1:
            return f"a static {name}_scale that is not one fp32 value"
        if zp is not None and (zp.dtype not in _QL_TYPE or zp.numel() != 1):
            return f"a static {name}_zero_point of {zp.numel()} x {zp.dtype} (one uint8 or int8 value has a kernel)"
    if bias is not None:
        b, b_scale, b_zp = bias
        if b.dtype != torch.int32 or b.numel() != n:
            return f"a bias of {b.numel()} x {b.dtype} (N int32 values)"
        if b_scale is None or b_scale.dtype != torch.float32 or b_scale.numel() != 1:
            return "a b_scale that is not one fp32 value"
        if b_zp is not None and (b_zp.dtype != torch.int32 or b_zp.numel() != 1):
            return f"a b_zero_point of {b_zp.numel()} x {b_zp.dtype} (one int32 value)"
    return None


def qdq_function(x: torch.Tensor, w: torch.Tensor, w_scale: torch.Tensor, w_zero_point: torch.Tensor | None = None, *, x_mode: str,
                 x_scale: torch.Tensor | None = None, x_zero_point: torch.Tensor | None = None, out_mode: str | None = None,
                 out_scale: torch.Tensor | None = None, out_zero_point: torch.Tensor | None = None, bias=None) -> torch.Tensor:
    """One call of a `quant`-domain QDQ function with quantized activations (`oq_qdq_function`, csrc/qdq_function.hip): the input
    Q -> DQ of ``x`` [..., K] fp32 (``x_mode`` "static": ``x_scale`` and ``x_zero_point``, whose type -- uint8 without one -- is the
    one ``x`` is quantized to; "dynamic": uint8 with DynamicQuantizeLinear's parameters of ``x``), the MatMul / Gemm against
    dequant(``w``) ([K, N] uint8 / int8, ``w_scale`` / ``w_zero_point`` per tensor or [N]), ``bias`` = (B int32 [N], b_scale,
    b_zero_point or None) dequantized and added, and the output Q -> DQ (``out_mode`` None, "static" or "dynamic").  fp32 [..., N]
    out.  The product is the exact int32 sum of (q_x - zp_x)(W - zp_w) on the int8 matrix cores; every parameter is a tensor on
    the device.  A NaN in ``x``: the bottom of the type under "static", every element of the result NaN under "dynamic".
    Deterministic; nothing synchronises with the host.

    NotImplementedError, naming the reason, for what the kernel leaves out (`qdq_function_unsupported`)."""
    b, b_scale, b_zp = bias if bias is not None else (None, None, None)
    named = dict(x=x, w=w, w_scale=w_scale, w_zero_point=w_zero_point, x_scale=x_scale, x_zero_point=x_zero_point, out_scale=out_scale,
                 out_zero_point=out_zero_point, B=b, b_scale=b_scale, b_zero_point=b_zp)
    for name, t in named.items():
        if t is not None:
            _require_device(t, name)
    why = qdq_function_unsupported(x, w, w_scale, w_zero_point, x_mode=x_mode, x_scale=x_scale, x_zero_point=x_zero_point, out_mode=out_mode,
                                   out_scale=out_scale, out_zero_point=out_zero_point, bias=bias)
    if why is not None:
        raise NotImplementedError(f"qdq_function: {why}")
    k, n = int(w.shape[0]), int(w.shape[1])
    rows = _rows_and_out(x.reshape(-1, k), n, torch.float32)
    if rows is None:
        return torch.zeros((*x.shape[:-1], n), dtype=torch.float32, device=x.device)
    x2, m, lda, out = rows
    w, ldw = _row_major(w)
    per_column = n > 1 and any(t is not None and t.numel() == n for t in (w_scale, w_zero_point))
    if per_column:      # one zero point for every column next to per-column scales (or the reverse): the library takes one code for both
        w_scale = w_scale.reshape(-1).expand(n) if w_scale.numel() == 1 else w_scale
        w_zero_point = w_zero_point.reshape(-1).expand(n) if w_zero_point is not None and w_zero_point.numel() == 1 else w_zero_point
    w_scale, w_zero_point, x_scale, x_zero_point, out_scale, out_zero_point, b, b_scale, b_zp = (
        None if t is None else t.contiguous() for t in (w_scale, w_zero_point, x_scale, x_zero_point, out_scale, out_zero_point, b, b_scale, b_zp))
    x_code, out_code = _QDQ_MODE[x_mode], _QDQ_MODE[out_mode]
    type_of = lambda zp: _QL_TYPE[torch.uint8 if zp is None else zp.dtype]      # noqa: E731
    lib = L.load()
    need = lib.oq_qdq_function_workspace_bytes(m, k, n, x_code, out_code)
    ws = _workspace(need, x.device)
    L.check(lib.oq_qdq_function(_ptr(x2), L.OQ_NBITS_F32, m, k, lda, x_code, type_of(x_zero_point), _ptr(x_scale), _ptr(x_zero_point), _ptr(w),
                                _QDQ_WTYPE[w.dtype], n, ldw, L.OQ_CHANNEL if per_column else L.OQ_TENSOR, 0, _ptr(w_scale), _ptr(w_zero_point),
                                _ptr(b), _ptr(b_scale), _ptr(b_zp), out_code, type_of(out_zero_point), _ptr(out_scale), _ptr(out_zero_point),
                                _ptr(out), n, _ptr(ws), need, _stream()))
    return out.reshape(*x.shape[:-1], n)


# ----------------------------------------------------------------------------- G1 - G4
def hessian_accumulate(x: torch.Tensor, h: torch.Tensor, n_seen: int, method: str | None = None) -> int:
    """gptq.py:246-260, in place on ``h`` [K, K]; ``x`` [n_add, ..., K] fp32, fp16 or bf16.  Returns the new sample
    count.  The activations are streamed through the MFMA TN GEMM; nothing is concatenated.  ``method``: the X^T X kernel
    of this call (None: the calling thread's default, `hessian_set_method`).

    An fp16 / bf16 ``x`` is read as it is (`oq_hessian_accumulate_h16`, csrc/syrk_bf16x3.hip section 4) and defines the result
    as gptq.py:257 does, on its exact fp32 values.  ``method`` and the thread default are IGNORED for it: half x half
    products are exact in fp32, so the one matrix-core product that route runs carries no operand split and no product
    rounding -- it is at least as exact as each of the fp32 methods, "f32" included, and there is nothing to choose."""
    _require_device(x, "x")
    half = x.dtype in _HALF_WTYPE
    if half:
        _method_code(method)                       # an unknown name is still an error
    else:
        _require_device(x, "x", torch.float32)
    _require_device(h, "H", torch.float32)
    n_add = int(x.shape[0])
    x2, ldx = _row_major(x.reshape(-1, x.shape[-1]))
    t, k = x2.shape
    if h.shape != (k, k) or not h.is_contiguous():
        raise ValueError(f"H must be a contiguous [{k}, {k}] tensor")
    lib = L.load()
    xargs, kind = _twin(x2)
    ws = _workspace(getattr(lib, _TWIN_WORKSPACE["hessian"][kind])(t, k), x.device)
    method_arg = () if half else (_method_code(method),)      # the `_h16` entry point has no such argument
    L.check(getattr(lib, "oq_hessian_accumulate_" + kind)(*xargs, t, k, ldx, int(n_seen), n_add, _ptr(h), *method_arg, _ptr(ws), ws.numel(), _stream()))
    return int(n_seen) + n_add


_MANY_MIN_K, _MANY_MIN_ROWS, _MANY_MAX_ROWS = 512, 512, 32768


def hessian_accumulate_many(xs, hs, n_seen) -> list[int]:
    """gptq.py:246-260 for a list of (input, Hessian) pairs -- the tensors one calibration batch taps -- in one launch chain per
    element type: `oq_hessian_accumulate_many_f32` for the fp32 items, `oq_hessian_accumulate_many_h16` for the fp16 items and
    again for the bf16 items, which are read as they are (no fp32 copy).  ``xs[i]`` [n_add, ..., K_i] fp32, fp16 or bf16,
    ``hs[i]`` [K_i, K_i] fp32 updated in place, ``n_seen[i]`` the samples already in it; returns the new sample counts.

    Items narrower than 512 columns or shorter than 512 rows (their padding to 256-wide tiles would cost more than the launches
    save) and items longer than 32 768 rows (a grouped product sums an item's rows in ONE fp32 chain; the per-tensor call slices
    long inputs, which also keeps the rounding error at 1e-6 of max |H|) go through `hessian_accumulate` one by one, whatever
    their type.  So does every fp32 item when another Hessian method than the fp16 pieces is selected; the method is irrelevant
    for half items (`hessian_accumulate`), which stay grouped.  A half type with a single eligible item takes the per-tensor call
    too: a chain of one saves no launch.  Grouped half items of up to 992 rows get the bits of `hessian_accumulate`, longer ones
    the same tolerance."""
    xs, hs, n_seen = list(xs), list(hs), [int(n) for n in n_seen]
    if not (len(xs) == len(hs) == len(n_seen)):
        raise ValueError("hessian_accumulate_many: xs, hs and n_seen must have one entry per item")
    out = [0] * len(xs)
    rows, keep = [], []
    half: dict = {}                   # element type -> [(index, table row, the tensor the row points into)]
    grouped = hessian_method() in ("auto", "f16x3")
    for i, (x, h) in enumerate(zip(xs, hs)):
        is_half = isinstance(x, torch.Tensor) and x.dtype in _HALF_WTYPE
        _require_device(x, "x", None if is_half else torch.float32)
        _require_device(h, "H", torch.float32)
        x2, ldx = _row_major(x.reshape(-1, x.shape[-1]))
        t, k = x2.shape
        if h.shape != (k, k) or not h.is_contiguous():
            raise ValueError(f"H[{i}] must be a contiguous [{k}, {k}] tensor")
        if not (grouped or is_half) or k < _MANY_MIN_K or t < _MANY_MIN_ROWS or t > _MANY_MAX_ROWS:
            out[i] = hessian_accumulate(x, h, n_seen[i])
            continue
        row = (x2.data_ptr(), h.data_ptr(), t, k, ldx, n_seen[i], int(x.shape[0]), 0)
        if is_half:
            half.setdefault(x.dtype, []).append((i, row, x2))
            continue
        rows.append(row)
        keep.append(x2)
        out[i] = n_seen[i] + int(x.shape[0])

    def launch(table, device, kind, *wtype):
        """One launch chain: the items ``table`` (64 bytes each) of one element type."""
        lib = L.load()
        _host, hp, dev = _item_table(table, device)
        ws = _workspace(getattr(lib, _TWIN_WORKSPACE["hessian_many"][kind])(hp, len(table)), device)
        L.check(getattr(lib, "oq_hessian_accumulate_many_" + kind)(hp, _ptr(dev), len(table), *wtype, _ptr(ws), ws.numel(), _stream()))

    if rows:
        launch(rows, keep[0].device, "f32")
    for dtype, items in half.items():
        if len(items) == 1:
            i = items[0][0]
            out[i] = hessian_accumulate(xs[i], hs[i], n_seen[i])
            continue
        launch([row for _, row, _ in items], items[0][2].device, "h16", _HALF_WTYPE[dtype])
        for i, row, _ in items:
            out[i] = row[5] + row[6]
    return out


class HessianPipeline:
    """gptq.py:246-260 for a SEQUENCE of batches, possibly of many inputs, with the two halves of every batch on two
    streams: the HBM-bound preparation (max |x|, scale, fp16 pieces: oq_hessian_prepare_f32) of batch i + 1 runs on a side
    stream while the matrix-core bound product of batch i (oq_hessian_accumulate_prepared_f32) runs on the caller's
    stream.  Two piece buffers, one slab buffer.  `accumulate(x, h, n_seen, next_x)` returns the new sample count like
    `hessian_accumulate`; `next_x` (the batch that will be accumulated next, for any H, or None) is prepared ahead.
    The results are bit-identical to `hessian_accumulate` with the fp16-piece method."""

    def __init__(self, device):
        self.device = device
        self.side = torch.cuda.Stream(device=device)
        self.bufs = [None, None]        # piece buffers
        self.ready = [None, None]       # event: pieces of the buffer are complete
        self.free = [None, None]        # event: the product that read the buffer is done
        self.tag = [None, None]         # (the prepared tensor itself, its ._version, shape, n_total): identity, not address
        self.slab = None
        self.slot = 0

    def reserve(self, rows: int, k: int) -> None:
        """Allocate the two piece buffers and the slab buffer for batches of up to `rows` x `k` now (otherwise on first use)."""
        lib = L.load()
        need = lib.oq_hessian_pieces_bytes(int(rows), int(k))
        for i in (0, 1):
            if self.bufs[i] is None or self.bufs[i].numel() < need:
                self.bufs[i] = torch.empty(need, dtype=torch.uint8, device=self.device)
        sl = lib.oq_hessian_slab_bytes(int(k))
        if self.slab is None or self.slab.numel() < sl:
            self.slab = torch.empty(sl, dtype=torch.uint8, device=self.device)

    @staticmethod
    def _flat(x):
        _require_device(x, "x", torch.float32)
        x2 = x.reshape(-1, x.shape[-1])
        return _row_major(x2)

    def _prepare(self, i, x, n_total):
        lib = L.load()
        x2, ldx = self._flat(x)
        t, k = x2.shape
        need = lib.oq_hessian_pieces_bytes(t, k)
        cur = torch.cuda.current_stream(self.device)
        if self.bufs[i] is None or self.bufs[i].numel() < need:
            old = self.bufs[i]
            if old is not None:
                # a prepare-ahead that was never consumed may still be writing the old buffer on the side stream, and a
                # product may still be reading it on the caller's: the block must not go back to the allocator (which
                # hands it out in the CALLER's stream order) before both are done
                old.record_stream(self.side)
                if self.ready[i] is not None:
                    cur.wait_event(self.ready[i])
            self.bufs[i] = torch.empty(need, dtype=torch.uint8, device=self.device)
            self.ready[i] = self.free[i] = self.tag[i] = None
        buf = self.bufs[i]
        off = (-buf.data_ptr()) % 256
        ev = torch.cuda.Event()
        ev.record(cur)                                  # X is ready on the caller's stream at this point
        with torch.cuda.stream(self.side):
            self.side.wait_event(ev)
            if self.free[i] is not None:
                self.side.wait_event(self.free[i])      # the product that read this buffer last
            L.check(lib.oq_hessian_prepare_f32(_ptr(x2), t, k, ldx, int(n_total), C.c_void_p(buf.data_ptr() + off), buf.numel() - off,
                                               C.c_void_p(self.side.cuda_stream)))
            done = torch.cuda.Event()
            done.record(self.side)
        x2.record_stream(self.side)
        self.ready[i] = done
        # the tag holds the tensor: while it is held its address cannot be handed to another batch by the allocator, and
        # `_version` catches an in-place edit between the preparation and the product
        self.tag[i] = (x2, x2._version, tuple(x2.shape), int(n_total))

    def accumulate(self, x, h, n_seen: int, next_x=None, next_n_total: int | None = None) -> int:
        lib = L.load()
        _require_device(h, "H", torch.float32)
        n_add = int(x.shape[0])
        x2, ldx = self._flat(x)
        t, k = x2.shape
        if h.shape != (k, k) or not h.is_contiguous():
            raise ValueError(f"H must be a contiguous [{k}, {k}] tensor")
        n_total = int(n_seen) + n_add
        i = self.slot
        tag = self.tag[i]
        # same storage (held by the tag, so its address cannot have been handed to another batch), same view, unedited
        prepared = (tag is not None and tag[0].untyped_storage().data_ptr() == x2.untyped_storage().data_ptr() and
                    tag[0].data_ptr() == x2.data_ptr() and tag[0].stride() == x2.stride() and tag[1] == x2._version and
                    tag[2] == tuple(x2.shape) and tag[3] == n_total)
        if not prepared:
            self._prepare(i, x, n_total)                # nothing (valid) was prepared ahead for this batch
        if next_x is not None:
            self._prepare(1 - i, next_x, next_n_total if next_n_total is not None else int(next_x.shape[0]))
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(self.ready[i])
        need = lib.oq_hessian_slab_bytes(k)
        if self.slab is None or self.slab.numel() < need:
            self.slab = torch.empty(need, dtype=torch.uint8, device=self.device)
        buf = self.bufs[i]
        off = (-buf.data_ptr()) % 256
        L.check(lib.oq_hessian_accumulate_prepared_f32(C.c_void_p(buf.data_ptr() + off), t, k, int(n_seen), n_add, _ptr(h), _ptr(self.slab),
                                                       self.slab.numel(), C.c_void_p(cur.cuda_stream)))
        fr = torch.cuda.Event()
        fr.record(cur)
        self.free[i] = fr
        self.tag[i] = None
        self.slot = 1 - i
        return n_total


HESSIAN_METHODS = {"auto": 0, "f32": 1, "bf16x6": 2, "bf16x9": 3, "f16x3": 4}
_METHOD_DEFAULT = threading.local()


def hessian_set_method(method: str) -> None:
    """The calling THREAD's default for the matrix-core products of the GPTQ path (include/oq_hip.h, G1): "auto" | "f32" |
    "bf16x6" | "bf16x9" | "f16x3".  A default provider only: the C library has no such state (ABI 2: the method is an
    argument of every entry point that uses it), and every function below also takes ``method=`` per call."""
    if method not in HESSIAN_METHODS:
        raise ValueError(f"unknown Hessian method {method!r}: one of {sorted(HESSIAN_METHODS)}")
    _METHOD_DEFAULT.value = method


def hessian_method() -> str:
    return getattr(_METHOD_DEFAULT, "value", "auto")


def _method_code(method: str | None) -> int:
    m = hessian_method() if method is None else method
    if m not in HESSIAN_METHODS:
        raise ValueError(f"unknown Hessian method {m!r}: one of {sorted(HESSIAN_METHODS)}")
    return HESSIAN_METHODS[m]


def gptq_prepare(w: torch.Tensor, h: torch.Tensor, actorder: bool):
    """gptq.py:118-127 in place on the working copies ``w`` [K, N] and ``h`` [K, K]; returns perm or None."""
    _require_device(w, "W", torch.float32)
    _require_device(h, "H", torch.float32)
    assert w.is_contiguous() and h.is_contiguous()
    k, n = w.shape
    lib = L.load()
    perm = torch.empty(k, dtype=torch.int32, device=w.device) if actorder else None
    ws = _workspace(lib.oq_gptq_prepare_workspace_bytes(k, n, int(actorder)), w.device)
    L.check(lib.oq_gptq_prepare_f32(_ptr(w), k, n, _ptr(h), int(actorder), _ptr(perm), _ptr(ws), ws.numel(), _stream()))
    return perm


def gptq_factor(h: torch.Tensor, percdamp: float, method: str | None = None):
    """gptq.py:134-150: returns (U [K, K] upper with inv(H + damp I) = U^T U, info int32[1] on device)."""
    _require_device(h, "H", torch.float32)
    assert h.is_contiguous() and h.dim() == 2 and h.shape[0] == h.shape[1]
    k = h.shape[0]
    lib = L.load()
    u = torch.empty((k, k), dtype=torch.float32, device=h.device)
    info = torch.zeros(1, dtype=torch.int32, device=h.device)
    ws = _workspace(lib.oq_gptq_factor_workspace_bytes(k), h.device)
    L.check(lib.oq_gptq_factor_f32(_ptr(h), k, float(percdamp), _ptr(u), _ptr(info), _method_code(method), _ptr(ws), ws.numel(), _stream()))
    return u, info


def gptq_factor_batched(h: torch.Tensor, percdamp: float, fix_dead: bool = False, method: str | None = None):
    """gptq.py:134-150 for a stack ``h`` [B, K, K] of Hessians of one width, factored in lock-step (one chain of
    launches for all of them).  Returns (U [B, K, K], info int32[B] on the device); matrix by matrix bit-identical to
    `gptq_factor`.  ``fix_dead``: zero diagonal entries count as 1 (gptq.py:119-120)."""
    _require_device(h, "H", torch.float32)
    if h.dim() != 3 or h.shape[1] != h.shape[2] or not h.is_contiguous():
        raise ValueError("H must be a contiguous [B, K, K] tensor")
    b, k = int(h.shape[0]), int(h.shape[1])
    lib = L.load()
    u = torch.empty((b, k, k), dtype=torch.float32, device=h.device)
    info = torch.zeros(b, dtype=torch.int32, device=h.device)
    ws = _workspace(lib.oq_gptq_factor_batched_workspace_bytes(k, b), h.device)
    L.check(lib.oq_gptq_factor_batched_f32(_ptr(h), k, k * k, b, float(percdamp), int(bool(fix_dead)), _ptr(u), k * k, _ptr(info),
                                           _method_code(method), _ptr(ws), ws.numel(), _stream()))
    return u, info


def gptq_shared_factors(h: torch.Tensor, percdamp: float, method: str | None = None):
    """`gptq_shared_factor` (no actorder) for a stack of Hessians [B, K, K]: one batched factor chain; returns the list
    of per-input dictionaries ``gptq_quantize(..., shared=...)`` takes (views into the batched results)."""
    u, info = gptq_factor_batched(h, percdamp, fix_dead=True, method=method)
    dead = torch.diagonal(h, dim1=1, dim2=2) == 0
    return [{"u": u[i], "info": info[i:i + 1], "perm": None, "dead": dead[i]} for i in range(h.shape[0])]


_LOOP_MODES = {"parity": L.OQ_GPTQ_PARITY, "corrected": L.OQ_GPTQ_CORRECTED, "corrected_columns": L.OQ_GPTQ_CORRECTED_COLUMNS}


def gptq_loop(w: torch.Tensor, u: torch.Tensor, qtype: str, group_size, symmetric: bool, reduce_range: bool,
              clip_ratio: float, mse: bool, block_size: int, mode: str, init_scale: torch.Tensor,
              init_zp: torch.Tensor, want_used: bool = False, layout: str = "kn", method: str | None = None):
    """gptq.py:153-216 on the working copy ``w`` (modified in place in corrected mode).
    Returns (q_int [K, N] or, with layout "kn_packed4", [K, N/2] nibble pairs; q_deq [K, N]; used_scale | None; used_zp | None).
    ``mode`` "corrected_columns" = "corrected" on the one-column-per-lane kernel (same bytes)."""
    _require_device(w, "W", torch.float32)
    _require_device(u, "U", torch.float32)
    assert w.is_contiguous() and u.is_contiguous()
    k, n = w.shape
    lib = L.load()
    g = int(group_size) if group_size else 0
    if layout not in ("kn", "kn_packed4"):
        raise ValueError("the GPTQ loop writes layout 'kn' or 'kn_packed4'")
    q_int = _q_buffer(layout, (), k, n, 0, qtype, w.device)
    q_deq = torch.empty((k, n), dtype=torch.float32, device=w.device)
    used_s = used_z = None
    if want_used and g > 0:
        ng = (k + g - 1) // g
        used_s = torch.empty((ng, n), dtype=torch.float32, device=w.device)
        used_z = torch.empty((ng, n), dtype=torch.int32, device=w.device)
    s0 = init_scale.to(torch.float32).contiguous().reshape(-1)
    z0 = init_zp.to(torch.int32).contiguous().reshape(-1)
    ws = _workspace(lib.oq_gptq_loop_workspace_bytes(k, n, int(block_size)), w.device)
    L.check(lib.oq_gptq_loop_f32(_ptr(w), k, n, _ptr(u), L.QTYPE_CODE[qtype], g, int(symmetric), int(reduce_range),
                                 float(clip_ratio), int(mse), int(block_size), _LOOP_MODES[mode], _method_code(method), _ptr(s0), _ptr(z0),
                                 s0.numel(), _ptr(q_int), _layout_code(layout), _ptr(q_deq), _ptr(used_s), _ptr(used_z), _ptr(ws),
                                 ws.numel(), _stream()))
    return q_int, q_deq, used_s, used_z


def gptq_shared_factor(h: torch.Tensor, percdamp: float, actorder: bool, method: str | None = None):
    """Everything of `_gptq` that depends on H only (gptq.py:118-150): the dead-channel mask, the optional
    actorder permutation and the inverse factor.  The reference recomputes this for every node; nodes that
    share an input (q/k/v, gate/up) share H, so one factor serves them all -- pass the result to
    ``gptq_quantize(..., shared=...)``."""
    _require_device(h, "H", torch.float32)
    k = h.shape[0]
    h1 = h.contiguous().clone()
    dummy = torch.zeros((k, 4), dtype=torch.float32, device=h.device)
    perm = gptq_prepare(dummy, h1, actorder)
    u, info = gptq_factor(h1, percdamp, method)
    dead = torch.diagonal(h) == 0
    return {"u": u, "info": info, "perm": perm, "dead": dead}


def gptq_quantize(w: torch.Tensor, h: torch.Tensor, qtype: str, strategy: str, group_size, symmetric=False,
                  reduce_range=False, clip_ratio=1.0, block_size=128, percdamp=0.01, actorder=False, mse=False,
                  mode: str = "parity", shared=None, layout: str = "kn", method: str | None = None):
    """gptq.py:76-243 (`_gptq`) on device tensors: ``w`` [K, N] weights, ``h`` [K, K] accumulated Hessian.
    Neither input is modified.  Returns (q_int, scale, zp, info) with the reference's output shapes; ``layout``
    "kn_packed4": q_int [K, N/2] as core/_pack.py:8-22 serialises the 4-bit result, written by the loop kernels.
    An fp16 / bf16 ``w`` takes one device cast, ``w.float()`` (exact): the arithmetic of GPTQ stays fp32."""
    if mode not in _LOOP_MODES:
        raise ValueError("mode must be 'parity' or 'corrected'")
    _require_device(w, "W")
    if w.dtype in _HALF_WTYPE:
        w = w.float()
    _require_device(w, "W", torch.float32)
    _require_device(h, "H", torch.float32)
    k, n = w.shape
    used = "channel" if strategy == "group" else strategy                      # gptq.py:92-96
    w1 = w.contiguous().clone()                                                  # :99-100
    h1 = h.contiguous().clone() if shared is None else None
    # :104-116 initial parameters: per out-channel over all of K (or global)
    _, s0, z0 = rtn_quantize(w1, qtype, used, -1, symmetric, reduce_range, clip_ratio, mse, emit_q=False)
    if shared is None:
        perm = gptq_prepare(w1, h1, actorder)                                    # :118-127
        u, info = gptq_factor(h1, percdamp, method)                              # :134-150
    else:   # H-only work done once for all layers with this input
        u, info, perm = shared["u"], shared["info"], shared["perm"]
        w1.masked_fill_(shared["dead"].unsqueeze(1), 0.0)                        # :121 (no host round trip, unlike w1[mask] = 0)
        if perm is not None:
            w1 = w1.index_select(0, perm.to(torch.int64)).contiguous()          # :126
    loop_g = group_size if (group_size and group_size != -1) else 0
    corrected_own = mode != "parity" and not actorder
    q_int, q_deq, us, uz = gptq_loop(w1, u, qtype, loop_g, symmetric, reduce_range, clip_ratio, mse, block_size,
                                     mode, s0, z0, want_used=corrected_own and strategy == "group", layout=layout, method=method)
    if actorder:                                                                 # :210-213
        inv = torch.argsort(perm.to(torch.int64))
        q_int = q_int.index_select(0, inv)
        q_deq = q_deq.index_select(0, inv)
    # :219-231 final parameters re-derived from the dequantized Q in the user's layout
    _, scale, zp = rtn_quantize(q_deq, qtype, strategy, group_size if group_size is not None else -1, symmetric,
                                reduce_range, clip_ratio, mse, emit_q=False)
    if corrected_own:
        g_eff = resolve_group("group", k, loop_g) if loop_g else 0
        if strategy == "group" and loop_g and k % g_eff == 0 and us is not None:
            # corrected mode returns the parameters the integers were produced with (see oracle/oq_oracle.py)
            scale = us.t().contiguous().reshape(-1, 1)
            zp = uz.t().contiguous().reshape(-1, 1).to(container_dtype(qtype))
        elif not loop_g and strategy in ("tensor", "channel"):
            scale, zp = s0.reshape(scale.shape), z0.reshape(zp.shape)
    return q_int, scale, zp, info
