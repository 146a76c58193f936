"""What the fp16-piece GEMM tests share (test_piece_gemm_cases.py, test_matmul_pieces_gpu.py): plain numpy, no library call.

`split`      the preparation restated (csrc/syrk_bf16x3.hip: absmax_scale_body<110>, row_pow2_scales_kernel, split_f16x2_body,
             split_f16x2_fast_axis_kernel): a power-of-two scale per row or per operand, hi = fp16(x s), lo = fp16(x s - hi);
`emulate`    the kernel's three products lo_a hi_b + hi_a lo_b + hi_a hi_b in float64, with the dropped lo_a lo_b and the `mass` every
             error term of the fp32 accumulation is a multiple of;
`exact_ok`   the conditions under which the kernel must return the float64 product bit for bit;
recipes      seeded integer operands that satisfy them;
`locate`     wrong output positions -> counts per slot of the kernel's tile, so that a failure reads
             "tile (1, 2), wm 3, wn 1, j 7, scalar store: 12 wrong" and not like a tensor diff.

Why integers come back exactly.  The scales are powers of two, so x s is exact; an integer of at most 22 bits splits into hi + lo
without loss; an fp16 x fp16 product is exact in fp32.  Every product of two pieces is then a multiple of u = u_a u_b, the product
of the lowest set bits of the two operands' pieces, and so is every partial sum, in whatever order the matrix instruction and the
stage loop add them.  A multiple of u below 2^24 u is an fp32 number.  Every partial sum is bounded by
mass = sum_k (|hi_a| + |lo_a|) (|hi_b| + |lo_b|); with mass < 2^24 u nothing is ever rounded.  The kernel leaves lo_a lo_b out, so
that term has to vanish.  The epilogue multiplies by the two inverse scales (powers of two) and by alpha and adds beta C: exact
again while |beta C| + |alpha| mass stays below 2^24 of THEIR common unit (`epilogue_ok`).

The representation bound.  With s = 2^(15 - ex) and m = f 2^ex the maximum the scale was taken from (the row's or the operand's),
0.5 <= f < 1, every |x s| <= 2^15.  hi = fp16(x s) is x s rounded to 11 significant bits; x s - hi is exact in fp32 and
lo = fp16(x s - hi) rounds it to 11 bits again: |x s - hi - lo| <= 2^-11 |x s - hi| <= 2^-22 |x s| -- unless lo falls below fp16's
normal range, where the error is half the last subnormal, 2^-25.  In x's units that is 2^-25 / s, and 1 / s = 2^(ex - 15) <= 2^-14 m
while the scale is not clamped, hence

    |x - (hi + lo) / s|  <=  2^-22 |x| + 2^-39 m                                     (include/oq_hip_nbits.h states the same)

and, with da, db these element errors,  |emulate - float64| <= sum_k (|da| |b| + |a| |db| + |lo_a| |lo_b| / (s_a s_b))  to first
order (`representation_bound`).  Where the clamp to 2^+-110 is reached (m below 2^-96) the second term is 2^-25 / s itself, which
is what `element_bound` returns; `scale_is_clamped` says where.

The summation bound.  The kernel and `emulate` hold the same pieces and add the same 3 * 32 * ceil(Kd / 32) products per output (32
per matrix instruction, three instructions per 32-row stage, zero padding included).  A sum of n fp32 terms in any order is off by at
most (n - 1) u / (1 - n u) < n u times the sum of the terms' magnitudes for n < 4096, u = 2^-24; the sum of the magnitudes is at
most `mass`.  The epilogue adds at most three roundings of the result (the two inverse scales, alpha), each 2^-24 of a value below
mass.  Hence  |kernel - emulate| <= (3 * 32 * ceil(Kd / 32) + 3) 2^-24 mass / (s_a s_b)  (`summation_bound`): below a dropped
piece's 2^-11 while Kd <= 512.
"""
import collections
import zlib

import numpy as np

TILE = 256                      # kST: a block's tile edge
STAGE_ROWS = 32                 # F16Stage::ROWS: contraction rows per stage (four chunks of 8)
HEADER_BYTES = 16384            # kScaleHeaderBytes: the scales and the absmax partials in front of the pieces


def ceil_div(a, b):
    return -(-a // b)


def pieces_bytes_at_least(Kd, cols):
    """What `matmul_pieces_layout` (csrc/gemm_tn.hip) takes: the pieces, the scale header, the row scales."""
    return ceil_div(Kd, STAGE_ROWS) * 4 * 2 * TILE * ceil_div(cols, TILE) * 16 + HEADER_BYTES + 8 * cols


# ------------------------------------------------------------------------------------ the preparation
def pow2_scale(m):
    """m: float32 maxima -> s = 2^(15 - ex) as float64, ex from frexp, clamped to 2^+-110; 1 for a zero or non-finite maximum."""
    m = np.asarray(m, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        _, ex = np.frexp(m)
        ok = (m > 0) & np.isfinite(m)
    e = np.clip(15 - ex.astype(np.int64), -110, 110)
    return np.where(ok, np.ldexp(1.0, np.where(ok, e, 0)), 1.0)


def scale_is_clamped(x, per_row):
    x = np.asarray(x, dtype=np.float32)
    m = np.abs(x).max(axis=-1, keepdims=True) if per_row else np.abs(x).max(keepdims=True)
    _, ex = np.frexp(m)
    return np.abs(15 - ex) > 110


def split(x, per_row):
    """x [rows, Kd] float32, the contraction on the last axis -> (hi, lo, s) as float64; s is [rows, 1] or [1, 1]."""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 2
    mag = np.abs(x)
    m = mag.max(axis=1, keepdims=True) if per_row else mag.max(keepdims=True).reshape(1, 1)      # NaN propagates, as nmax does
    s = pow2_scale(m)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        xs = x * s.astype(np.float32)                                  # a power of two: exact
        hi = xs.astype(np.float16)                                     # round to nearest even
        lo = (xs - hi.astype(np.float32)).astype(np.float16)           # the difference is exact in fp32
    return hi.astype(np.float64), lo.astype(np.float64), s


def lowest_set_bit(*pieces):
    """The lowest set bit over the given pieces, per row ([rows, 1] float64); 1 for a row of zeros.  Finite fp16 values are
    multiples of 2^-24 below 2^16: as integers they fit an int64."""
    out = None
    for p in pieces:
        q = np.round(p * 2.0 ** 24).astype(np.int64)
        assert np.array_equal(q.astype(np.float64), p * 2.0 ** 24)
        bit = (q & -q).astype(np.float64)
        bit[bit == 0] = np.inf
        row = bit.min(axis=1, keepdims=True)
        out = row if out is None else np.minimum(out, row)
    out[np.isinf(out)] = 2.0 ** 24
    return out / 2.0 ** 24


Emulated = collections.namedtuple("Emulated", "y lolo mass units s_a s_b lossless")


def emulate(a, b, per_row_a):
    """a [M, Kd], b [Kd, N] float32.  y: the three products in float64 with the scales taken out again; lolo: the dropped
    lo_a lo_b, in y's units; mass [M, N]: sum_k (|hi_a| + |lo_a|) (|hi_b| + |lo_b|) in the pieces' units; units: mass in units of the
    product of the lowest set bits of a's row and b's column; s_a [M, 1] (or [1, 1]), s_b [1, 1]; lossless: hi + lo == x s for
    every element of both operands."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    ha, la, sa = split(a, per_row_a)
    hb, lb, sb = split(b.T, False)
    hb, lb = hb.T, lb.T
    with np.errstate(invalid="ignore", over="ignore"):
        unscale = 1.0 / (sa * sb)
        y = (la @ hb + ha @ lb + ha @ hb) * unscale
        lolo = (la @ lb) * unscale
        mass = (np.abs(ha) + np.abs(la)) @ (np.abs(hb) + np.abs(lb))
        lossless = bool(np.array_equal(ha + la, a.astype(np.float64) * sa) and np.array_equal(hb + lb, b.astype(np.float64) * sb))
    if np.isfinite(mass).all():
        units = mass / (lowest_set_bit(ha, la) * lowest_set_bit(hb.T, lb.T).T)
    else:
        units = np.full_like(mass, np.inf)
    return Emulated(y, lolo, mass, units, sa, sb, lossless)


def exact_ok(a, b, per_row_a):
    """The kernel must return float64(a) @ float64(b) bit for bit, in whatever order the matrix instruction adds: nothing is
    lost in the split (integers of at most 22 bits), the dropped lo_a lo_b is zero everywhere, and mass < 2^24 units everywhere."""
    em = emulate(a, b, per_row_a)
    return bool(em.lossless and not em.lolo.any() and em.units.max() < 2.0 ** 24)


def epilogue_ok(a, b, per_row_a, alpha, beta, c):
    """The same for C = beta C + alpha A B on INTEGER operands (unit 1): beta C and alpha A B are multiples of one power of two
    u, and |beta C| + |alpha| sum |a| |b| < 2^24 u."""
    a64, b64, c64 = (np.asarray(t, dtype=np.float64) for t in (a, b, c))
    assert all(np.array_equal(t, np.round(t)) for t in (a64, b64, c64))
    terms = np.concatenate([np.abs(beta * c64).ravel(), [abs(alpha)]])
    terms = terms[terms > 0]
    mant, _ = np.frexp(terms)
    q = np.round(mant * 2.0 ** 53).astype(np.int64)                  # the significand as an integer
    u = (terms / mant * (q & -q).astype(np.float64) * 2.0 ** -53).min()
    total = np.abs(beta * c64) + abs(alpha) * (np.abs(a64) @ np.abs(b64))
    return bool(exact_ok(a, b, per_row_a) and total.max() < 2.0 ** 24 * u)


# ------------------------------------------------------------------------------------ the bounds
def element_bound(x, per_row):
    """|x - (hi + lo) / s| allowed per element: 2^-22 |x| + 2^-25 / s (= at most 2^-39 m while the scale is not clamped)."""
    x = np.asarray(x, dtype=np.float64)
    _, _, s = split(x.astype(np.float32), per_row)
    return 2.0 ** -22 * np.abs(x) + 2.0 ** -25 / s


def representation_bound(a, b, per_row_a):
    """|emulate - float64| allowed per output element (module docstring)."""
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    _, la, sa = split(np.asarray(a, dtype=np.float32), per_row_a)
    _, lb, sb = split(np.asarray(b, dtype=np.float32).T, False)
    da, db = element_bound(a64, per_row_a), element_bound(b64.T, False).T
    return da @ np.abs(b64) + np.abs(a64) @ db + (np.abs(la) @ np.abs(lb.T)) / (sa * sb)


def summation_bound(em, Kd):
    """|kernel - emulate| allowed per output element (module docstring)."""
    return (3 * STAGE_ROWS * ceil_div(Kd, STAGE_ROWS) + 3) * 2.0 ** -24 * em.mass / (em.s_a * em.s_b)


# ------------------------------------------------------------------------------------ the exact recipes
def _rng(name, M, Kd, N):
    return np.random.default_rng([zlib.crc32(name.encode()), M, Kd, N])


def _integers(r, bound, shape):
    return r.integers(-bound, bound + 1, size=shape).astype(np.float32)


def a_two_pieces(M, Kd, N):
    """A: integers in +-4100 (13 bits: the odd ones above 2048 need a lo); B: integers in +-3."""
    r = _rng("a_two_pieces", M, Kd, N)
    return _integers(r, 4100, (M, Kd)), _integers(r, 3, (Kd, N))


def b_two_pieces(M, Kd, N):
    """The mirror image: A in +-3, B in +-4100."""
    r = _rng("b_two_pieces", M, Kd, N)
    return _integers(r, 3, (M, Kd)), _integers(r, 4100, (Kd, N))


def both_two_pieces(M, Kd, N):
    """Both operands with two pieces, never at the same k: at even k A is in +-4100 and B in +-3, at odd k the other way round.
    lo_a lo_b vanishes term by term, while lo . hi AND hi . lo are live in every slot of every tile (with `a_two_pieces` alone a
    hi . lo product that is wrong somewhere multiplies zeros)."""
    r = _rng("both_two_pieces", M, Kd, N)
    a, b = _integers(r, 3, (M, Kd)), _integers(r, 3, (Kd, N))
    a[:, 0::2] = _integers(r, 4100, a[:, 0::2].shape)
    b[1::2] = _integers(r, 4100, b[1::2].shape)
    return a, b


def one_piece(M, Kd, N):
    """A: integers in +-1500, B: integers in +-5: every lo is zero."""
    r = _rng("one_piece", M, Kd, N)
    return _integers(r, 1500, (M, Kd)), _integers(r, 5, (Kd, N))


def full_width(M, Kd, N, per_column=7):
    """A: odd integers up to 2^21 - 1, all 22 bits of the two pieces in use, row 0 at +-(2^21 - 1) throughout (|hi| + |lo| is
    2^21 + 1 units there); B: `per_column` entries of +-1 in every column (as many as Kd has), the rest 0.  Seven is the most
    mass < 2^24 allows: 8 (2^21 + 1) > 2^24."""
    r = _rng("full_width", M, Kd, N)
    top = 2 ** 21 - 1
    a = r.integers(0, 2 ** 20, size=(M, Kd)) * 2 + 1
    a[0] = top
    a = (a * r.choice([-1, 1], size=(M, Kd))).astype(np.float32)
    b = np.zeros((Kd, N), dtype=np.float32)
    for n in range(N):
        rows = r.choice(Kd, size=min(per_column, Kd), replace=False)
        b[rows, n] = r.choice([-1.0, 1.0], size=len(rows))
    return a, b


RECIPES = {f.__name__: f for f in (a_two_pieces, b_two_pieces, both_two_pieces, one_piece, full_width)}


def integer_c(M, N):
    """A C for the beta != 0 calls: even integers in +-2000, so that beta = 0.5 leaves integers."""
    return (np.arange(M * N).reshape(M, N) % 2001 * 2.0 - 2000.0).astype(np.float32)


def beyond_2048_rows(which):
    """The absmax partition (make_f16x2_pieces: min(rows, 2048) blocks of ceil(rows / blocks) rows) on a source of 2081 rows, recipe
    `one_piece`, the single largest element -- a power of two -- in the LAST source row.  A maximum taken without that row gives a
    scale under which the element overflows fp16.  -> (a, b, per_row_a)
      "b": a k-major B [2081, 8] with 2048 in its last row (without it: s = 2^12, 2048 s = 2^23);
      "a": a fast-axis A [2081, 8] under the operand's scale with 2^17 in its last row (without it: s = 2^4, 2^21)."""
    if which == "b":
        a, b = one_piece(2081, 2081, 8)
        b[2080, 3] = 2048.0
        return a, b, True
    a, b = one_piece(2081, 8, 8)
    a[2080, 5] = 2.0 ** 17
    return a, b, False


# the (recipe, (M, Kd, N), per_row_a) triples of test_matmul_pieces_gpu.py: test_piece_gemm_cases.py checks every one
TILE_GRID = [(1, 1), (1, 257), (255, 4), (256, 256), (257, 513), (300, 130), (64, 129), (513, 3)]         # (M, N) at Kd = 100
CONTRACTIONS = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 96, 97, 1000]                                          # Kd at (M, N) = (70, 37)
FORMS_SHAPE = (70, 100, 37)
STORE_N = (36, 37, 38, 39)
GUARD_SHAPES = [(1, 1, 1), (70, 33, 37), (257, 97, 300)]
GRID_RECIPES = ("a_two_pieces", "both_two_pieces")          # of the tile grid and the contraction edges


def exact_cases():
    cases = [(name, (M, 100, N), True) for M, N in TILE_GRID for name in GRID_RECIPES]
    cases += [(name, (70, Kd, 37), True) for Kd in CONTRACTIONS for name in GRID_RECIPES]
    cases += [(name, (70, 1000, 37), True) for name in RECIPES]
    cases += [(name, FORMS_SHAPE, per_row) for name in ("a_two_pieces", "b_two_pieces") for per_row in (True, False)]
    cases += [("a_two_pieces", (70, 100, N), True) for N in STORE_N]
    cases += [("a_two_pieces", shape, per_row) for shape in GUARD_SHAPES for per_row in (True, False)]
    cases += [("one_piece", FORMS_SHAPE, per_row) for per_row in (True, False)]
    return sorted(set(cases))


# ------------------------------------------------------------------------------------ the random cases (magnitudes)
MAGNITUDE_SHAPES = [(70, 300, 37), (260, 512, 40)]
MAGNITUDES = ["plain", "a 1e-30", "a 1e30", "b 1e-30", "b 1e30", "rows 1e9 apart", "one element 2^18 above its row"]


def magnitude_case(kind, shape, seed=0):
    """Random operands, not exact: -> (a, b) float32."""
    M, Kd, N = shape
    r = np.random.default_rng([zlib.crc32(kind.encode()), M, Kd, N, seed])
    a = r.standard_normal((M, Kd)) * np.exp(r.uniform(-1, 1, size=(M, 1)))
    b = r.standard_normal((Kd, N)) / 32
    if kind.startswith("a 1e"):
        a = a * float(kind[2:])
    elif kind.startswith("b 1e"):
        b = b * float(kind[2:])
    elif kind == "rows 1e9 apart":
        a = a * (10.0 ** (9 * (np.arange(M) % 3 - 1)))[:, None]
    elif kind == "one element 2^18 above its row":
        rows = np.arange(0, M, 3)
        cols = r.integers(0, Kd, size=len(rows))
        a[rows, cols] = np.abs(a[rows]).max(axis=1) * 2.0 ** 18
    else:
        assert kind == "plain", kind
    return a.astype(np.float32), b.astype(np.float32)


def magnitude_cases():
    return [(kind, shape, per_row) for kind in MAGNITUDES for shape in MAGNITUDE_SHAPES for per_row in (True, False)]


# ------------------------------------------------------------------------------------ where a wrong output sits in the tile
Slot = collections.namedtuple("Slot", "tile_m tile_n wm wn i j kc cl store last_group")


def _fields(wrong_mask, ldc, aligned):
    mask = np.asarray(wrong_mask, dtype=bool)
    M, N = mask.shape
    row, col = np.nonzero(mask)
    vec_ok = (N if ldc is None else ldc) % 4 == 0 and aligned
    last_group = col // 4 * 4 + 3 >= N                                # `col + 3 < N` is false for the lane's first column
    vector = vec_ok & ~last_group
    return np.stack([row // 256, col // 256, row % 256 // 64, col % 256 // 128, row % 64 // 16, col % 128 // 16, row % 16 // 4, col % 16,
                     vector.astype(np.int64), last_group.astype(np.int64)], axis=1)


def _named(f):
    return Slot(*(int(v) for v in f[:8]), "vector" if f[8] else "scalar", bool(f[9]))


def locate(wrong_mask, ldc=None, aligned=True):
    """wrong_mask [M, N] bool -> {Slot: count}.  The kernel's map (gemm_f16x3_body, f16_m16_mainloop, staged_tile_epilogue): a block
    owns the 256 x 256 tile (tile_m, tile_n) = (row // 256, col // 256); wave (wm, wn) of its 4 x 2 owns rows wm * 64 ... (also
    the epilogue's pass) and columns wn * 128 ...; there MFMA tile (i, j) is 16 x 16; in it the lane holds rows 4 kc ... 4 kc + 3 of
    column cl.  store: the epilogue's lane writes its four columns as one vector where ldc % 4 == 0, the base of C is 16-byte
    aligned (`aligned`) and all four lie inside N; last_group: the column is in its row's last, partial group of four (N % 4 != 0)."""
    fields = _fields(wrong_mask, ldc, aligned)
    slots, counts = np.unique(fields, axis=0, return_counts=True) if len(fields) else (fields, [])
    return {_named(f): int(k) for f, k in zip(slots, counts)}


def compact(values):
    """[0, 1, 2, 3, 7] -> '[0-3, 7]'."""
    values = [int(v) for v in values]
    runs, start = [], 0
    for i in range(1, len(values) + 1):
        if i == len(values) or values[i] != values[i - 1] + 1:
            runs.append(str(values[start]) if i - 1 == start else f"{values[start]}-{values[i - 1]}")
            start = i
    return "[" + ", ".join(runs) + "]"


def describe(wrong_mask, ldc=None, aligned=True, most=6):
    """`locate` as text: the number of wrong outputs, per coordinate the values that occur among them, and the (tile, wave, j, store
    form) groups hit most, each as "tile (1, 2), wm 3, wn 1, j 7, scalar store: 12 wrong"."""
    fields = _fields(wrong_mask, ldc, aligned)
    if not len(fields):
        return "no mismatch"
    names = Slot._fields
    parts = [f"{names[k]} {compact(np.unique(fields[:, k]))}" for k in range(8)]
    coarse, counts = np.unique(fields[:, [0, 1, 2, 3, 5, 8]], axis=0, return_counts=True)
    order = np.argsort(-counts, kind="stable")[:most]
    worst = "; ".join(f"tile ({c[0]}, {c[1]}), wm {c[2]}, wn {c[3]}, j {c[4]}, {'vector' if c[5] else 'scalar'} store: {int(counts[o])} wrong"
                      for o, c in ((o, coarse[o]) for o in order))
    partial = int(fields[:, 9].sum())
    return (f"{len(fields)} wrong in {len(coarse)} groups ({partial} in a row's last group of four): " + ", ".join(parts) + " -- " + worst)
