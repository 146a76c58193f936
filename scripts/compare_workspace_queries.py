#!/usr/bin/env python3
"""What do the `*_workspace_bytes` queries of two builds of liboq_hip.so return?  No GPU is needed: a query is host arithmetic.

    python scripts/compare_workspace_queries.py PARENT/onnx_quantize_amd/lib/liboq_hip.so onnx_quantize_amd/lib/liboq_hip.so [--markdown]

Every size query of the library over a table of shapes: the ones bench.py, bench_gptq.py and bench_calib.py use, the small ones
of the ABI tests, and one per bound that makes a query answer 0.  Rule per row: `=` where a header states the formula or a test
pins the value (or a relation between two values, listed at the end), `<=` everywhere else -- a workspace a caller sized with the
parent's query must still be large enough.  Exit status 1 if a rule is broken.
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys

import numpy as np

GROUP, CHANNEL, TENSOR = 2, 1, 0       # oq_strategy
HUGE = 1 << 62
I64, I32, PTR = C.c_int64, C.c_int32, C.c_void_p


def hessian_items(shapes):
    """oq_hessian_item: int64 {X, H, T, K, ldx, n_seen, n_add, 0}; the queries read T and K only"""
    return np.array([[4096, 8192, t, k, k, 0, t, 0] for t, k in shapes], dtype=np.int64)


def stats_items(shapes):
    """oq_abs_stats_item: {X, T, K, ldx, abs_sum, absmax}"""
    return np.array([[4096, t, k, k, 8192, 12288] for t, k in shapes], dtype=np.int64)


# (query, argument types, rule, [argument tuples]); a numpy table argument is passed as (pointer, rows)
ROWS = [
    ("oq_matmul_nbits_workspace_bytes", [I64, I64, I64, I64, I32], "=",
     [(16, 512, 128, 32, 0), (16, 512, 128, 32, 1), (1, 4096, 4096, 128, 0), (2048, 4096, 4096, 128, 1), (33, 100, 7, 32, 0), (0, 64, 64, 32, 0)]),
    ("oq_qlinear_matmul_workspace_bytes", [I64, I64, I64], "=", [(16, 512, 128), (1, 4096, 4096), (2048, 4096, 4096), (33, 100, 7), (0, 64, 64)]),
    ("oq_hessian_half_workspace_bytes", [I64, I64], "=", [(64, 32), (33, 257), (65536, 4096), (65536, 11008), (0, 32), (64, 1 << 18)]),
    ("oq_hessian_many_half_workspace_bytes", "hessian_items", "=", [((64, 32),) * 3, ((2048, 4096), (2048, 11008)), ((0, 32),)]),
    ("oq_minmax_half_workspace_bytes", [I64], "=", [(1,), (1 << 40,), (0,)]),
    ("oq_minmax_many_half_workspace_bytes", [I64], "=", [(1,), (72,), (65535,), (0,), (65536,)]),
    ("oq_absmax_half_workspace_bytes", [I64, I64, I32], "=", [(64, 32, 0), (129, 33, 0), (129, 33, 1), (4096, 11008, 0), (0, 32, 0)]),
    ("oq_abs_stats_many_half_workspace_bytes", "stats_items", "=", [((64, 40), (64, 72)), ((2048, 4096), (2048, 11008)), ((0, 40),)]),
    ("oq_rtn_mse_half_workspace_bytes", [I64, I64, I32, I64], "=", [(256, 64, GROUP, 128), (4096, 11008, GROUP, 128), (256, 64, TENSOR, -1), (256, 64, GROUP, 96)]),
    ("oq_rtn_half_workspace_bytes", [I64, I64, I32, I64], "<=", [(256, 64, CHANNEL, -1), (4096, 11008, GROUP, 512), (256, 64, GROUP, 128), (0, 64, CHANNEL, -1)]),
    ("oq_rtn_workspace_bytes", [I64, I64, I32, I64, I32], "<=",
     [(4096, 11008, GROUP, 128, 0), (4096, 11008, GROUP, 128, 1), (4096, 11008, CHANNEL, -1, 0), (4096, 11008, TENSOR, -1, 0), (256, 64, GROUP, 128, 1),
      (256, 64, TENSOR, -1, 1), (4096, 4096, GROUP, 512, 0), (33, 72, CHANNEL, -1, 1), (0, 64, GROUP, 128, 0), (256, 64, GROUP, 96, 0)]),
    ("oq_rtn_state_bytes", [I64, I64, I32, I64], "<=",
     [(4096, 11008, GROUP, 128), (4096, 4096, GROUP, 64), (4096, 11008, CHANNEL, -1), (4096, 11008, TENSOR, -1), (333, 77, TENSOR, -1), (0, 64, GROUP, 128)]),
    ("oq_rtn_batched_workspace_bytes", [I64, I64, I64, I64], "<=", [(8, 4096, 11008, 128), (3, 256, 64, 128), (1, 4096, 4096, 32), (0, 256, 64, 128), (65536, 256, 64, 128)]),
    ("oq_rtn_tensor_many_workspace_bytes", [I64], "<=", [(1,), (72,), (65535,), (0,)]),
    ("oq_hessian_workspace_bytes", [I64, I64], "<=", [(65536, 4096), (65536, 11008), (2048, 4096), (64, 32), (33, 257), (0, 32)]),
    ("oq_hessian_many_workspace_bytes", "hessian_items", "<=", [((64, 32),) * 3, ((2048, 4096), (2048, 11008)), ((0, 32),)]),
    ("oq_hessian_pieces_bytes", [I64, I64], "<=", [(65536, 4096), (2048, 11008), (64, 32), (0, 32)]),
    ("oq_hessian_slab_bytes", [I64], "<=", [(4096,), (11008,), (32,), (0,)]),
    ("oq_matmul_pieces_bytes", [I64, I64], "<=", [(4096, 4096), (4096, 11008), (100, 7), (0, 7)]),
    ("oq_gptq_prepare_workspace_bytes", [I64, I64, I32], "<=", [(4096, 4096, 1), (11008, 4096, 1), (192, 64, 1), (4096, 4096, 0), (0, 64, 1)]),
    ("oq_gptq_factor_workspace_bytes", [I64], "<=", [(4096,), (11008,), (192,), (128,), (0,), (1 << 18,)]),
    ("oq_gptq_factor_batched_workspace_bytes", [I64, I64], "<=", [(4096, 1), (4096, 4), (11008, 4), (192, 3), (4096, 0), (4096, 65536)]),
    ("oq_gptq_loop_workspace_bytes", [I64, I64, I64], "<=",
     [(4096, 4096, 128), (4096, 11008, 128), (11008, 4096, 128), (256, 64, 128), (256, 64, 256), (300, 37, 64), (4096, 4096, 1024), (0, 64, 128), (256, 64, 0)]),
    ("oq_hqq_workspace_bytes", [I64, I64, I64], "<=", [(4096, 11008, 128), (4096, 4096, 64), (128, 64, 64), (128, 64, -1), (100, 37, 20), (128, 64, 48), (0, 64, 64)]),
    ("oq_awq_workspace_bytes", [I64, I64, I64], "<=", [(96, 256, 64), (1, 4, 1), (48, 1100, 256), (4096, 4096, 4096), (480, 160, 7), (16384, 4096, 11008), (0, 64, 8), (16, 65536, 8)]),
    ("oq_awq_half_workspace_bytes", [I64, I64, I64], "<=", [(96, 256, 64), (1, 4, 1), (48, 1100, 256), (4096, 4096, 4096), (480, 160, 7), (0, 64, 8)]),
    ("oq_awq_stats_workspace_bytes", [I64, I64], "<=", [(256, 64), (4, 1), (1100, 256), (4096, 4096), (4096, 11008), (0, 8)]),
    ("oq_awq_stats_half_workspace_bytes", [I64, I64], "<=", [(256, 64), (4, 1), (1100, 256), (4096, 4096), (0, 8)]),
    ("oq_abs_sum_cols_workspace_bytes", [I64], "<=", [(4096,), (11008,), (37,), (0,)]),
    ("oq_smooth_quant_workspace_bytes", [I64], "<=", [(4096,), (11008,), (37,), (0,)]),
    ("oq_minmax_workspace_bytes", [I64], "<=", [(1,), (1 << 30,)]),
    ("oq_minmax_many_workspace_bytes", [I64], "<=", [(1,), (72,), (65535,), (0,)]),
    ("oq_absmax_workspace_bytes", [I64, I64, I32], "<=", [(64, 32, 0), (129, 33, 0), (129, 33, 1), (4096, 11008, 0), (0, 32, 0)]),
]
TABLES = {"hessian_items": hessian_items, "stats_items": stats_items}


def query(lib, name, types, args):
    fn = getattr(lib, name)
    fn.restype = C.c_size_t
    if isinstance(types, str):
        table = TABLES[types](args)
        fn.argtypes = [PTR, I64]
        return fn(C.c_void_p(table.ctypes.data), len(table))
    fn.argtypes = types
    return fn(*args)


def relations(lib):
    """the relations between two values that tests pin (test_awq_half_abi.py, test_mse_half_abi.py, test_library_abi.py)"""
    out = []
    for t, k, n in ((96, 256, 64), (1, 4, 1), (48, 1100, 256), (4096, 4096, 4096), (480, 160, 7)):
        r = -(-8 * n * (-(-k // 64) + k // 257 + 1) // 256) * 256 + 256
        out.append((f"awq half - fp32 = R  T={t} K={k} N={n}",
                    query(lib, "oq_awq_half_workspace_bytes", [I64] * 3, (t, k, n)) - query(lib, "oq_awq_workspace_bytes", [I64] * 3, (t, k, n)) == r))
        out.append((f"awq stats half - fp32 = R  K={k} N={n}",
                    query(lib, "oq_awq_stats_half_workspace_bytes", [I64] * 2, (k, n)) - query(lib, "oq_awq_stats_workspace_bytes", [I64] * 2, (k, n)) == r))
    for k, n, s, g in ((512, 520, GROUP, 128), (1024, 257, GROUP, -1), (4096, 11008, CHANNEL, -1), (33, 72, TENSOR, -1)):
        types = [I64, I64, I32, I64, I32]
        diff = query(lib, "oq_rtn_workspace_bytes", types, (k, n, s, g, 1)) - query(lib, "oq_rtn_workspace_bytes", types, (k, n, s, g, 0))
        out.append((f"rtn mse=1 - mse=0 = mse half  K={k} N={n}", diff == query(lib, "oq_rtn_mse_half_workspace_bytes", types[:4], (k, n, s, g))))
    one, four = query(lib, "oq_gptq_factor_workspace_bytes", [I64], (4096,)), query(lib, "oq_gptq_factor_batched_workspace_bytes", [I64, I64], (4096, 4))
    out.append(("factor batched(K, 1) = factor(K)", query(lib, "oq_gptq_factor_batched_workspace_bytes", [I64, I64], (4096, 1)) == one))
    out.append(("|factor batched(K, 4) - 4 factor(K)| < 16384", abs(four - 4 * one) < 16384))
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("change")
    ap.add_argument("--markdown", action="store_true", help="print the table as markdown")
    a = ap.parse_args()
    parent, change = C.CDLL(a.parent), C.CDLL(a.change)
    bad = 0
    if a.markdown:
        print("| query | arguments | rule | parent | change |\n|---|---|---|---:|---:|")
    for name, types, rule, cases in ROWS:
        for args in cases:
            p, c = query(parent, name, types, args), query(change, name, types, args)
            ok = p == c if rule == "=" else c <= p
            bad += not ok
            shown = ", ".join("x".join(map(str, x)) if isinstance(x, tuple) else ("2^62" if x == HUGE else str(x)) for x in args)
            line = f"| `{name}` | {shown} | {rule} | {p} | {c} |" if a.markdown else f"{name}({shown}): {rule}  parent {p}  change {c}"
            print(line + ("" if ok else "   <-- BROKEN"))
    for side, lib in (("parent", parent), ("change", change)):
        for what, ok in relations(lib):
            bad += not ok
            if not ok or not a.markdown:
                print(f"{side}: {what}: {'holds' if ok else 'BROKEN'}")
    print(f"{sum(len(r[3]) for r in ROWS)} queries compared, {bad} broken")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
