"""What the fp32-activation Hessian tests share (test_hessian_cases.py, test_hessian_exact_gpu.py): plain numpy, no library call.

H = beta H + alpha X^T X for X [T, K] fp32 (oq_hessian_accumulate_f32, csrc/gemm_tn.hip) under its four arithmetic methods:
  f32     gemm_tn_kernel on fl32(x sx), sx = fl32(sqrt(2 / n)), alpha = 1;
  bf16x9  x = hi + mid + lo in bf16 (split_bf16x3_kernel), all nine piece products, alpha = fl32(2 / n);
  bf16x6  the six products of TermSeq<6> (lo.lo, lo.mid and mid.lo are dropped);
  f16x3   s = 2^(15 - ex) from the batch maximum, hi = f16(x s), lo = f16(x s - hi), hi.hi + hi.lo + lo.hi, alpha / s^2.

`split_bf16x3`, `split_f16x2_hessian`   the preparations restated from the code;
`kept_sum`, `expected`                  the products a method keeps, in float64, and the epilogue (fl32(alpha v), then
                                        fl32(fl32(beta old) + that): the library is built with -ffp-contract=off);
`exact_ok`                              where the kernel must return `expected` bit for bit, whatever the order of its sums;
recipes                                 seeded operands that satisfy it;  `slices_of`  the T-slice choice restated;
`locate`, `describe`                    wrong output positions -> tile, wave, triangle and store arm.

Why bits come back.  A piece product is exact in fp32 (8 x 8 or 11 x 11 bits; for f32 the matrix instruction is a fused
multiply-add).  Every product of piece p of column i with piece q of column j is a multiple of lsb_p(i) lsb_q(j), the lowest set
bits over the columns' pieces; with u the smallest of these units over the KEPT (p, q) that meet anything, every partial sum, in
any order, is a multiple of u and bounded by mass = sum |a| |b| over the kept products.  mass < 2^24 u: nothing is ever rounded.
(piece_gemm_cases.exact_ok takes one unit per operand and asks the dropped lo.lo to vanish.  Here the dropped products must NOT
vanish -- the recipes have to tell the methods apart -- and they are what carries the lowest bits: the unit is taken per kept
pair.)  The epilogue is exact when each of its three roundings is, which is checked on the float64 values.

What cannot be exact.  An element with s significant bits has a square of at least 2 s - 1, so the diagonal of a column that
holds an element with all three bf16 pieces (s >= 18) is no fp32 number under a method that keeps every product (f32, bf16x9);
neither is an off-diagonal element in which two such elements meet.  `exact_ok(...).mask` leaves exactly those out for these two
methods (they are held to `summation_bound` instead); for bf16x6 and f16x3 the dropped products take the low bits away and
every element is exact.

A zero sum is +0.0: the accumulators start at +0.0, x + (-x) is +0.0 under round-to-nearest, alpha > 0, and h0 holds no -0.0.
`expected` adds +0.0 for that; the kernels' output is compared as it is.
"""
import collections
import math
import zlib

import numpy as np

from piece_gemm_cases import ceil_div, compact

METHODS = ("f32", "bf16x6", "bf16x9", "f16x3")
METHOD_CODE = {"auto": 0, "f32": 1, "bf16x6": 2, "bf16x9": 3, "f16x3": 4}            # include/oq_hip.h
PRODUCTS = {"f32": 1, "bf16x6": 6, "bf16x9": 9, "f16x3": 3}
# TermSeq<6>, TermSeq<9> (0 = hi, 1 = mid, 2 = lo) and f16_m16_mainloop's lo.hi, hi.lo, hi.hi (0 = hi, 1 = lo)
TERMS = {"f32": [(0, 0)],
         "bf16x6": list(zip((2, 0, 1, 1, 0, 0), (0, 2, 1, 0, 1, 0))),
         "bf16x9": list(zip((2, 2, 1, 2, 0, 1, 1, 0, 0), (2, 1, 2, 0, 2, 1, 0, 1, 0))),
         "f16x3": [(1, 0), (0, 1), (0, 0)]}
TILE = {"f32": 128, "bf16x6": 256, "bf16x9": 256, "f16x3": 256}                    # kBM; kST
STAGE_ROWS = {"f32": 32, "bf16x6": 16, "bf16x9": 16, "f16x3": 32}                  # kBT; Bf16Stage::ROWS; F16Stage::ROWS
HEADER_BYTES = 16384                                                                # kScaleHeaderBytes
SCALE_CLAMP = 60                                                                    # absmax_scale_body<60>


def fl32(v):
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------ the host's scalars
def alpha_of(n_total):
    return float(np.float32(2.0 / float(n_total)))


def beta_of(n_seen, n_total):
    return 0.0 if n_seen == 0 else float(np.float32(float(n_seen) / float(n_total)))


def sx_of(n_total):
    return float(np.float32(math.sqrt(2.0 / float(n_total))))


def is_pow2(v):
    return v > 0 and math.frexp(v)[0] == 0.5


# ------------------------------------------------------------------------------------ the preparations
def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even) as float32; finite input."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split_bf16x3(x):
    """split_pair: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid); the subtractions are exact.  -> float64 each."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16_round(x)
    r = x - hi
    mid = bf16_round(r)
    lo = bf16_round(r - mid)
    return hi.astype(np.float64), mid.astype(np.float64), lo.astype(np.float64)


def batch_scale(x):
    """absmax_scale_body<60>: s = 2^(15 - ex), max |x| = f 2^ex with f in [0.5, 1), the exponent clamped to +-60; 1 for an
    all-zero or non-finite batch."""
    m = np.float32(np.abs(np.asarray(x, dtype=np.float32)).max()) if np.size(x) else np.float32(0)
    if not (m > 0 and np.isfinite(m)):
        return 1.0
    e = 15 - int(np.frexp(m)[1])
    return float(np.ldexp(1.0, max(-SCALE_CLAMP, min(SCALE_CLAMP, e))))


def split_f16x2_hessian(x, alpha):
    """split_f16x2_body under the batch scale: -> (hi, lo, s), float64.  hi = f16(x s), lo = f16(x s - hi) (the difference is
    exact in fp32), and the dead-channel guard: where fl32(fl32(x x) alpha) > 0 and hi came out as +-0, hi keeps one unit
    (+-2^-24).  lo is taken from the unguarded hi."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    s = batch_scale(x)
    with np.errstate(over="ignore", under="ignore"):
        xs = x * np.float32(s)                                         # a power of two: exact (s <= 2^60 keeps it finite)
        hi = xs.astype(np.float16)
        lo = (xs - hi.astype(np.float32)).astype(np.float16)
        alive = ((x * x) * np.float32(alpha)) > 0 if alpha > 0 else np.zeros(x.shape, dtype=bool)
    bits = hi.view(np.uint16).copy()
    fire = alive & ((bits & 0x7FFF) == 0)
    bits[fire] |= 1
    return bits.view(np.float16).astype(np.float64), lo.astype(np.float64), s


def pieces_of(method, x, n_total):
    """-> (pieces as float64 arrays, what the accumulator has to be divided by: s^2 or 1)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if method == "f32":
        return [(x * np.float32(sx_of(n_total))).astype(np.float64)], 1.0        # store_piece: one fp32 rounding per element
    if method in ("bf16x6", "bf16x9"):
        return list(split_bf16x3(x)), 1.0
    hi, lo, s = split_f16x2_hessian(x, alpha_of(n_total))
    return [hi, lo], s * s


def kept_sum(method, x, n_total=2):
    """The products the method keeps, summed in float64 and with the batch scale taken out: what alpha multiplies."""
    pieces, div = pieces_of(method, x, n_total)
    v = sum(pieces[p].T @ pieces[q] for p, q in TERMS[method])
    return v / div


def epilogue(method, v, n_seen, n_add, h0=None):
    """fl32(alpha v), then fl32(fl32(beta old) + that); alpha is 1 for f32 (2 / n sits in sx).  -> float32"""
    n = n_seen + n_add
    alpha = 1.0 if method == "f32" else alpha_of(n)
    beta = beta_of(n_seen, n)
    out = fl32(alpha * fl32(v))
    if beta != 0.0:
        out = fl32(fl32(beta * np.asarray(h0, dtype=np.float64)) + out)
    return (out + 0.0).astype(np.float32)                                    # a zero is +0.0 (module docstring)


def expected(method, x, n_seen=0, n_add=2, h0=None):
    return epilogue(method, kept_sum(method, x, n_seen + n_add), n_seen, n_add, h0)


# ------------------------------------------------------------------------------------ exactness
def _lsb(v):
    """lowest set bit of every element of a float64 array (inf for a zero)."""
    mant, ex = np.frexp(v)
    q = np.round(np.abs(mant) * 2.0 ** 53).astype(np.int64)
    low = (q & -q).astype(np.float64)
    out = np.ldexp(low, ex - 53)
    out[q == 0] = np.inf
    return out


def _column_lsb(p):
    return _lsb(p).min(axis=0) if p.shape[0] else np.full(p.shape[1], np.inf)


def _pair_units(pa, pb):
    """u [K, K]: a power of two that divides every product pa[t, i] pb[t, j] (inf where all are zero).  Rows with at most four
    entries (the wide recipes): the smallest lsb(pa[t, i]) lsb(pb[t, j]) over the rows where both are live; otherwise the
    product of the columns' lowest set bits, which is no larger."""
    K = pa.shape[1]
    la, lb = _lsb(pa), _lsb(pb)
    most = int(max((pa != 0).sum(axis=1).max(initial=0), (pb != 0).sum(axis=1).max(initial=0)))
    if most > 4:
        return _column_lsb(pa)[:, None] * _column_lsb(pb)[None, :]
    u = np.full((K, K), np.inf)
    ia, ib = np.argsort(pa == 0, axis=1, kind="stable")[:, :most], np.argsort(pb == 0, axis=1, kind="stable")[:, :most]
    t = np.arange(pa.shape[0])
    for a in range(ia.shape[1]):
        for b in range(ib.shape[1]):
            i, j = ia[:, a], ib[:, b]
            val = la[t, i] * lb[t, j]
            live = np.isfinite(val)
            np.minimum.at(u, (i[live], j[live]), val[live])
    return u


Exact = collections.namedtuple("Exact", "mask all lossless mass units epilogue_exact")


def mass_of(method, x, n_total=2):
    """-> (mass [K, K] = sum |a| |b| over the kept products, u [K, K] = their smallest unit), in the pieces' own scale."""
    pieces, _ = pieces_of(method, x, n_total)
    K = x.shape[1]
    mass = np.zeros((K, K))
    unit = np.full((K, K), np.inf)
    mags = [np.abs(p) for p in pieces]
    for p, q in TERMS[method]:
        mass += mags[p].T @ mags[q]
        unit = np.minimum(unit, _pair_units(pieces[p], pieces[q]))
    return mass, unit


def exact_ok(method, x, n_seen=0, n_add=2, h0=None):
    """Where the kernel must return `expected` bit for bit (module docstring).  lossless: the pieces add up to x (x s) wherever
    the dead-channel guard has not fired -- the guard's unit is part of what is multiplied, not a loss."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = n_seen + n_add
    pieces, div = pieces_of(method, x, n)
    if method == "f32":
        lossless = bool(np.array_equal(pieces[0], x.astype(np.float64) * sx_of(n)))
    elif method == "f16x3":
        s = math.sqrt(div)
        guard = (np.abs(pieces[0]) == 2.0 ** -24) & (np.abs(x.astype(np.float64) * s) < 2.0 ** -24)
        lossless = bool(np.array_equal((pieces[0] + pieces[1])[~guard], (x.astype(np.float64) * s)[~guard]))
    else:
        lossless = bool(np.array_equal(sum(pieces), x.astype(np.float64)))
    mass, unit = mass_of(method, x, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        units = np.where(mass > 0, mass / unit, 0.0)
    v = kept_sum(method, x, n)
    alpha = 1.0 if method == "f32" else alpha_of(n)
    beta = beta_of(n_seen, n)
    a = alpha * v
    steps = (fl32(v) == v) & (fl32(a) == a)
    if beta != 0.0:
        b = beta * np.asarray(h0, dtype=np.float64)
        steps &= (fl32(b) == b) & (fl32(a + b) == a + b)
    with np.errstate(invalid="ignore"):
        finite = np.isfinite(a) & ((a == 0) | (np.abs(a) >= 2.0 ** -126))
    mask = (units < 2.0 ** 24) & steps & finite & lossless
    return Exact(mask, bool(mask.all()), lossless, mass, units, steps)


def summation_bound(method, x, n_seen, n_add, slices, h0=None):
    """|kernel - expected| allowed per element on any data.  The sum: one fp32 rounding per accumulated product (zero padding
    included), per slice addition, for alpha and for the final add, hence (products * padded_rows + slices + 3) 2^-24 sum |a| |b|
    over the kept products, in H's units.  The old H only meets two roundings, fl32(beta old) and the final add:
    2 * 2^-24 |beta h0| (times 1 + 2^-23 for the second-order term) -- it does not widen the bound of the sum."""
    n = n_seen + n_add
    mass, _ = mass_of(method, x, n)
    _, div = pieces_of(method, x, n)
    alpha = 1.0 if method == "f32" else alpha_of(n)
    padded_rows = ceil_div(x.shape[0], STAGE_ROWS[method]) * STAGE_ROWS[method]
    bound = (PRODUCTS[method] * padded_rows + slices + 3) * 2.0 ** -24 * (alpha * mass / div)
    if n_seen:
        bound = bound + 2.0 * 2.0 ** -24 * (1.0 + 2.0 ** -23) * beta_of(n_seen, n) * np.abs(np.asarray(h0, dtype=np.float64))
    return bound


# ------------------------------------------------------------------------------------ the recipes
def _rng(name, T, K):
    return np.random.default_rng([zlib.crc32(name.encode()), T, K])


def small_integers(T, K):
    """Integers in +-8: one piece under every method."""
    return _rng("small_integers", T, K).integers(-8, 9, size=(T, K)).astype(np.float32)


def _wide(name, T, K, low_of, e_min, e_max, headroom, meet=True):
    """A sparse X whose column j lives at one power of two 2^e_j: plain entries +-2^e_j and WIDE entries +-(2^e_j + low_of(e_j)).
    Rows carry two entries (one where K = 1): in every 8-row chunk -- in every row while the columns stay short -- a wide one at
    column c and a partner at another column, plain in even wide rows (exact under every method) and wide in odd ones (two
    multi-piece elements meet: the dropped products are live OFF the diagonal too; never with `meet` false).  e_j is as large as
    the column's entry count allows: count * 2^e_j units must stay below 2^24."""
    r = _rng(name, T, K)
    step = 1 if 2 * T <= 16 * K else 8
    rows = np.arange(0, T, step)
    rows = np.minimum(rows + (np.arange(len(rows)) % step), T - 1)
    idx = np.arange(len(rows))
    c = (5 * idx + 1) % K
    p = (c + 1 + idx % max(K - 1, 1)) % K
    count = np.bincount(np.concatenate([c, p]) if K > 1 else c, minlength=K)
    e = np.clip(headroom - np.ceil(np.log2(np.maximum(count, 1))).astype(np.int64), e_min, e_max)
    x = np.zeros((T, K), dtype=np.float64)
    sign = r.choice([-1.0, 1.0], size=(len(rows), 2))
    x[rows, c] = sign[:, 0] * (2.0 ** e[c] + low_of(e[c], idx))
    if K > 1:
        wide_partner = (idx % 2 == 1) & meet
        x[rows, p] = sign[:, 1] * (2.0 ** e[p] + np.where(wide_partner, low_of(e[p], idx + 1), 0.0))
    out = x.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), x)
    return out


def two_pieces(T, K):
    """12 to 22 significant bits: wide entries 2^e + 1 or + 3, e in 11 .. 21 -- hi and lo of the fp16 split, hi and mid (from e = 8
    on) of the bf16 split."""
    return _wide("two_pieces", T, K, lambda e, i: 1.0 + 2.0 * (i % 2), 11, 21, 21)


def two_pieces_low(T, K):
    """`two_pieces` at e = 11 throughout: 2049^2 = 2^22 + 2^12 + 1 is an fp32 number, so the dropped lo.lo survives the rounding of the
    result and the bits of f16x3 differ from those of f32 (at the widths of `two_pieces` they only differ before it)."""
    return _wide("two_pieces_low", T, K, lambda e, i: 1.0 + 2.0 * (i % 2), 11, 11, 21)


def mid_pairs(T, K):
    """9 to 12 significant bits, wide entries 2^e + 1 or + 3 with e in 8 .. 11, as small as the columns' entry counts ask: hi and mid
    of the bf16 split (lo is zero), and in odd wide rows two such entries meet, so that mid.mid, hi.mid and mid.hi are live off the
    diagonal too.  A square has at most 23 bits: every element is an fp32 number under EVERY method, the diagonal included -- the
    recipe on which the four middle products of bf16x9 are compared on bits."""
    return _wide("mid_pairs", T, K, lambda e, i: 1.0 + 2.0 * (i % 2), 8, 11, 11)


def three_pieces(T, K):
    """18 to 24 significant bits: wide entries 2^e + 2^(e - 9) + 1, e in 17 .. 23: hi = 2^e, mid = 2^(e - 9), lo = 1.  (2^(e - 8)
    would be a tie of the first rounding; with 17 bits, 2^16 + 2^7 + 1, the last bit still fits mid.)"""
    return _wide("three_pieces", T, K, lambda e, i: 2.0 ** (e - 9) + 1.0, 17, 23, 22)


def three_pieces_apart(T, K):
    """`three_pieces` in which no two wide entries share a row: every off-diagonal element is an fp32 number under the methods
    that keep every product as well; only the diagonal of a column with a wide entry is not (module docstring)."""
    return _wide("three_pieces_apart", T, K, lambda e, i: 2.0 ** (e - 9) + 1.0, 17, 23, 22, meet=False)


def scaled(e):
    def recipe(T, K):
        return (small_integers(T, K).astype(np.float64) * 2.0 ** e).astype(np.float32)
    recipe.__name__ = f"scaled({e})"
    return recipe


def guarded(T, K):
    """small integers with column 1 at +-2^-42 (2^-45 below the maximum 8: under fp16's last subnormal after the scaling, its
    squares 2^-84 alive in fp32), column 2 dead and column 3 all -0.0.  K >= 5; the maximum 8 is planted in column 0."""
    assert K >= 5
    x = small_integers(T, K)
    x[0, 0] = 8.0
    x[:, 1] = np.where(x[:, 1] < 0, -1.0, 1.0) * np.float32(2.0 ** -42)
    x[:, 2] = 0.0
    x[:, 3] = -0.0
    return x


def maximum_last(T, K):
    """small integers with the single largest element, 1024, in the last row and last column: a maximum taken without that row
    (the absmax partition: min(T, 2048) blocks of ceil(T / blocks) rows; 256 blocks in the grouped chain) gives a scale under
    which it overflows fp16."""
    x = small_integers(T, K)
    x[T - 1, K - 1] = 1024.0
    return x


def outlier_channels(T, K):
    """The input of test_hessian_f16_pieces_are_scale_free at reduced size: normal samples, channels 1e5 apart, one dead.  Not exact."""
    r = _rng("outlier_channels", T, K)
    chan = np.exp(r.uniform(np.log(1e-3), np.log(1e2), size=K)).astype(np.float32)
    x = r.standard_normal((T, K)).astype(np.float32) * chan
    if K > 7:
        x[:, 7] = 0
    return x


def normal(T, K):
    return _rng("normal", T, K).standard_normal((T, K)).astype(np.float32)


RECIPES = {f.__name__: f for f in (small_integers, two_pieces, two_pieces_low, mid_pairs, three_pieces, three_pieces_apart, guarded, maximum_last, outlier_channels, normal,
                                   scaled(-50), scaled(0), scaled(50))}
WIDEST = {"f32": "three_pieces_apart", "bf16x6": "three_pieces", "bf16x9": "three_pieces_apart", "f16x3": "two_pieces"}
def recipes_of(method):
    """What every line of the GPU grid runs for a method."""
    return ("small_integers", WIDEST[method], "mid_pairs")


KEEPS_EVERYTHING = ("f32", "bf16x9")         # their kept sum IS the product: the mask may leave out what no fp32 number holds


def integer_h0(x, K):
    """A symmetric integer H for the running-average calls: -8, -4, 0, 4 or 8 times m_i m_j, m_i the leading power of two of column
    i's maximum over 8 (at least 1; 1 for a zero column).  beta in {1/2, 3/4} leaves multiples of m_i m_j, which the kept sums of
    the recipes are too (their low bits sit far enough up: `exact_ok` checks the three roundings)."""
    m = np.abs(np.asarray(x, dtype=np.float64)).max(axis=0) if len(x) else np.zeros(K)
    lead = np.where(m > 0, np.ldexp(1.0, np.frexp(np.where(m > 0, m, 1.0))[1] - 1), 1.0)
    m = np.maximum(np.floor(lead / 8.0), 1.0) if m.max(initial=0) >= 1 else np.where(m > 0, lead / 8.0, 1.0)
    i, j = np.meshgrid(np.arange(K), np.arange(K), indexing="ij")
    base = ((np.minimum(i, j) * 7 + np.maximum(i, j) * 3) % 5 - 2) * 4.0
    out = (base * m[:, None] * m[None, :]).astype(np.float32)
    assert np.array_equal(out, out.T)
    return out


# ------------------------------------------------------------------------------------ the T-slices
def padded_k(K):
    return ceil_div(K, 256) * 256


def pieces_bytes(T, K):
    """syrk_bf16x3_pieces_bytes: room for either kind of pieces and the scale header."""
    b16 = ceil_div(T, 16) * 2 * 3
    f16 = ceil_div(T, 32) * 4 * 2
    return max(b16, f16) * padded_k(K) * 16 + HEADER_BYTES


def pieces_workspace_bytes(T, K, slab_bytes=0):
    """syrk_bf16x3_workspace_bytes: the pieces, the slabs, one alignment unit (workspace.hpp)."""
    return ceil_div(pieces_bytes(T, K), 256) * 256 + ceil_div(slab_bytes, 4) * 4 + 256


def slab_bytes_in(method, T, K, workspace_bytes):
    """What a call finds for slabs in a workspace of that many bytes: all of it for f32 (the slabs lie at the caller's pointer),
    what is left behind the pieces and the alignment unit for the piece methods."""
    if method == "f32":
        return workspace_bytes
    return max(0, workspace_bytes - ceil_div(pieces_bytes(T, K), 256) * 256 - 256) // 4 * 4


Slices = collections.namedtuple("Slices", "count per last")     # per, last: stages (f32: rows) of a slice and of the last one


def slices_of(method, T, K, slab_bytes):
    if method == "f32":                                          # launch_syrk_tn
        tn = ceil_div(K, 128)
        tiles = tn * (tn + 1) // 2
        splits = 1
        if slab_bytes > 0 and tiles < 8 * 512:
            splits = min(ceil_div(8 * 512, tiles), max(T // 256, 1), 16)
            while splits > 1 and splits * K * K * 4 > slab_bytes:
                splits -= 1
        if splits <= 1:
            return Slices(1, T, T)
        per = ceil_div(ceil_div(T, splits), 32) * 32
        splits = ceil_div(T, per)
        return Slices(splits, per, T - (splits - 1) * per)
    rows = STAGE_ROWS[method]                                    # choose_t_slices, then the re-division of syrk_pieces_phases
    nstages = ceil_div(T, rows)
    tn = padded_k(K) // 256
    tiles = tn * (tn + 1) // 2
    cap = min(max(nstages // (512 // rows), 1), 16)
    while cap > 1 and cap * K * K * 4 > slab_bytes:
        cap -= 1
    best, splits = -1.0, 1
    for c in range(1, cap + 1):
        blocks = tiles * c
        fill = blocks / (ceil_div(blocks, 256) * 256)
        if fill > best + 0.02:
            best, splits = fill, c
    per = ceil_div(nstages, splits)
    splits = ceil_div(nstages, per)
    return Slices(splits, per, nstages - (splits - 1) * per)


def first_split_rows(method, K, slab_bytes=1 << 62):
    """The smallest T that `slices_of` cuts."""
    step = STAGE_ROWS[method] if method != "f32" else 1
    T = 1
    while slices_of(method, T, K, slab_bytes).count == 1:
        T += step
        assert T < 1 << 20
    while T > 1 and slices_of(method, T - 1, K, slab_bytes).count > 1:
        T -= 1
    return T


# ------------------------------------------------------------------------------------ where a wrong element sits
Place = collections.namedtuple("Place", "tile_m tile_n wm wn triangle store")


def _places(wrong_mask, method, K, sliced, aligned):
    mask = np.asarray(wrong_mask, dtype=bool)
    row, col = np.nonzero(mask)
    r, c = np.minimum(row, col), np.maximum(row, col)            # the element the kernel computed: the upper one
    tile = TILE[method]
    tri = np.where(col > row, 0, np.where(col < row, 1, 2))      # upper, mirrored, diagonal
    if method == "f32":                                          # 2 x 2 waves, each rows {32 w .. } and {64 + 32 w ..}
        wm, wn = r % 64 // 32, c % 64 // 32
    else:                                                        # 4 x 2 waves of 64 x 128
        wm, wn = r % 256 // 64, c % 256 // 128
    # store arm: the reduction of a sliced call and the bf16 / fp32 epilogues store scalars; syrk_tile_store writes a lane's four
    # columns as one vector where K % 4 == 0, H is 16-byte aligned, all four lie inside K and, in a diagonal tile, none lies left
    # of the diagonal; the lower triangle is always a scalar mirror
    group = c // 4 * 4
    vector = (method == "f16x3") & (not sliced) & (K % 4 == 0) & aligned & (group + 3 < K) & ~((r // tile == c // tile) & (group < r)) & (tri != 1)
    return np.stack([r // tile, c // tile, wm, wn, tri, np.asarray(vector, dtype=np.int64)], axis=1) if len(row) else np.zeros((0, 6), dtype=np.int64)


_TRIANGLE = ("upper", "mirrored", "diagonal")


def locate(wrong_mask, method, K, sliced=False, aligned=True):
    """wrong_mask [K, K] bool -> {Place: count}: the block's tile (256, or 128 for f32) and wave that computed the element -- for
    one below the diagonal, its mirror image --, the triangle it lies in and the store arm that wrote it."""
    f = _places(wrong_mask, method, K, sliced, aligned)
    slots, counts = np.unique(f, axis=0, return_counts=True) if len(f) else (f, [])
    return {Place(int(s[0]), int(s[1]), int(s[2]), int(s[3]), _TRIANGLE[s[4]], "vector" if s[5] else "scalar"): int(k) for s, k in zip(slots, counts)}


def describe(wrong_mask, method, K, sliced=False, aligned=True, most=6):
    f = _places(wrong_mask, method, K, sliced, aligned)
    if not len(f):
        return "no mismatch"
    names = ("tile_m", "tile_n", "wm", "wn")
    parts = [f"{names[k]} {compact(np.unique(f[:, k]))}" for k in range(4)]
    parts.append("triangle " + "/".join(_TRIANGLE[t] for t in np.unique(f[:, 4])))
    slots, counts = np.unique(f, axis=0, return_counts=True)
    order = np.argsort(-counts, kind="stable")[:most]
    worst = "; ".join(f"tile ({s[0]}, {s[1]}), wm {s[2]}, wn {s[3]}, {_TRIANGLE[s[4]]}, {'vector' if s[5] else 'scalar'} store: {int(counts[o])} wrong"
                      for o, s in ((o, slots[o]) for o in order))
    return f"{len(f)} wrong of {K * K} ({method}, {'sliced' if sliced else 'direct'}): " + ", ".join(parts) + " -- " + worst


# ------------------------------------------------------------------------------------ the cases of test_hessian_exact_gpu.py
CONTRACTION_T = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 65]        # at K = 40
WIDTH_K = [1, 3, 4, 127, 128, 129, 255, 256, 257, 260, 513]                  # at T = 33
NINE_COLUMNS = {"f32": 1100, "bf16x6": 2052, "bf16x9": 2052, "f16x3": 2052}  # at T = 40
FORMS_SHAPE = (33, 260)
N_TOTALS = [(0, 2), (1, 1), (6, 2), (16, 16)]                                # (n_seen, n_add)
FULL = 1 << 62                                                               # a slab budget that never binds
# (T, K) -> the slice count a full workspace gives; test_hessian_cases.py proves every entry
SLICE_SHAPES = {
    "f32": {(511, 40): 1, (512, 40): 2, (513, 40): 2, (1000, 40): 3, (4096, 40): 16},
    "bf16x6": {(1008, 520): 1, (1009, 520): 2, (1521, 300): 3, (1553, 300): 3},
    "bf16x9": {(1008, 520): 1, (1009, 520): 2, (1521, 300): 3, (1553, 300): 3},
    "f16x3": {(992, 520): 1, (993, 520): 2, (1505, 300): 3, (1537, 300): 3},
}
RUNNING_SHAPES = {"f32": [(33, 260), (33, 257), (513, 40)], "bf16x6": [(33, 260), (33, 257), (1009, 520)],
                  "bf16x9": [(33, 260), (33, 257), (1009, 520)], "f16x3": [(33, 260), (33, 257), (993, 520)]}
SCALE_SHAPE = (2081, 40)
AUTO_SHAPES = [(8, 2048), (8, 2047)]
PREPARED_SHAPES = [(33, 40), (993, 520), (40, 2052)]
GROUPED_ITEMS = [(1, 1), (33, 257), (513, 40), (40, 520), (65, 256), (32, 2052)]      # (T, K); n_seen, ldx: grouped_table
TOLERANCE_SHAPES = {"f32": [(33, 260), (1000, 40), (512, 256)], "bf16x6": [(33, 260), (1009, 520), (512, 256)],
                    "bf16x9": [(33, 260), (1009, 520), (512, 256)], "f16x3": [(33, 260), (993, 520), (512, 256)]}


def grouped_table():
    """(T, K, ldx, n_seen, n_add, recipe) per item of the grouped call."""
    seen = [(0, 2), (1, 1), (6, 2), (0, 8), (16, 16), (0, 2)]
    recipes = ["small_integers", "two_pieces", "maximum_last", "two_pieces", "small_integers", "small_integers"]
    return [(T, K, K + 1 if i == 1 else K, *seen[i], recipes[i]) for i, (T, K) in enumerate(GROUPED_ITEMS)]


def exact_cases():
    """Every (method, recipe, T, K, n_seen, n_add) that test_hessian_exact_gpu.py compares on bits."""
    cases = set()
    for m in METHODS:
        both = recipes_of(m)
        cases |= {(m, r, T, 40, 0, 2) for T in CONTRACTION_T for r in both}
        cases |= {(m, r, 33, K, 0, 2) for K in WIDTH_K for r in both}
        cases |= {(m, r, 40, NINE_COLUMNS[m], 0, 2) for r in both}
        cases |= {(m, r, *FORMS_SHAPE, 0, 2) for r in both}
        cases |= {(m, r, T, K, 0, 2) for (T, K) in SLICE_SHAPES[m] for r in both}
        cases |= {(m, r, T, K, ns, na) for (T, K) in RUNNING_SHAPES[m] for ns, na in N_TOTALS for r in both}
    cases |= {("f16x3", f"scaled({e})", *SCALE_SHAPE, 0, 2) for e in (-50, 0, 50)}
    cases |= {("f16x3", "guarded", *SCALE_SHAPE, 0, 2), ("f16x3", "maximum_last", *SCALE_SHAPE, 0, 2)}
    cases |= {("f16x3", "two_pieces_low", 8, 2048, 0, 2), ("f32", "two_pieces_low", 8, 2047, 0, 2), ("f32", "two_pieces_low", 8, 2048, 0, 2)}
    cases |= {("f16x3", r, T, K, 0, 2) for (T, K) in PREPARED_SHAPES for r in ("small_integers", "two_pieces")}
    cases |= {("f16x3", r, T, K, ns, na) for (T, K, _, ns, na, r) in grouped_table()}
    return sorted(cases)
