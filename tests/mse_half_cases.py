"""The oracle case of the half-precision MSE search, shared by tests/test_mse_half_abi.py (CPU: the input's undecided share) and
tests/test_mse_half_gpu.py (GPU: the verdict): 256 x 192 standard normal values rounded to the element type, uint4, groups of 64
and 256.  An ordinary module."""
import numpy as np

ORACLE_SHAPE = (256, 192)
ORACLE_GROUPS = (64, 256)
# Seeds chosen on the CPU (0, 1, 2, .. tried in order, the first one kept) so that tests/mse_verdict.py, from the oracle's
# arithmetic alone, leaves at most 1 % of the rows undecided at BOTH group sizes: 7 of 768 rows at g = 64, 1 of 192 at g = 256.
# fp16: seed 0 leaves 1 and 2 rows, seed 1 leaves 0 and 1.  bf16: seed 0 leaves 1 and 0.
ORACLE_SEED = {"float16": 1, "bfloat16": 0}


def round_to(w, dtype):
    """fp32 array -> the nearest value of `dtype` (ties to even), as fp32.  Finite inputs well inside the type's range."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    if dtype == "float16":
        return w.astype(np.float16).astype(np.float32)
    u = w.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(w.shape)


def oracle_matrix(dtype):
    return round_to(np.random.default_rng(ORACLE_SEED[dtype]).standard_normal(ORACLE_SHAPE, dtype=np.float32), dtype)


def undecided_rows(w, g):
    """(rows the reference alone leaves undecided, rows, tables, judgement) of the uint4 group case."""
    import mse_verdict as V
    t = V.tables(w, "uint4", "group", g, False, False)
    j = V.judge(t)
    return int((~j.decided & ~t.nan_rows).sum()), t.e32.shape[1], t, j
