"""Inputs, launch plans and failure reports for the exact tests of the group-strategy RTN kernels (csrc/rtn.hip:
`rtn_group_wave<8|16|32>`, their five-waves-per-SIMD builds, `rtn_group_wave_pair`, `rtn_group_fused`).  NumPy and the oracle
only: tests/test_rtn_group_cases.py checks on the host that every case of tests/test_rtn_group_exact_gpu.py is the test it
claims to be.

Why these inputs.  The kernels compute rint(x * fl(1/s)) and trust it only when it is farther than `thr` from a half-integer
(`make_colq`, csrc/oq_common.hpp); otherwise a wave-uniform ballot redoes the rows with the IEEE division.  On i.i.d. normal
weights rint(x * fl(1/s)) and the oracle's rint(fl(x / s)) agree on every element of a million, so a band that is too narrow
or taken from the wrong column, a fallback that reads another column's scale and a redo of the wrong row are all invisible.
`boundary_dense` puts every element within two ulp of a rounding boundary of its own (column, k-group) grid, and on none of the
exact ties of the fast path's own arithmetic (a residual of 0.5 fires the redo whatever the band is): one element in thirty
then differs between the two formulas, every level is used, and every row of every strip holds such an element, so that
every ballot fires because of the band.  docs/LAB_NOTES_r46.md has the figures and the mutants these tests were held to."""
from __future__ import annotations

import functools
import warnings
from dataclasses import dataclass

import numpy as np

import oq_oracle as O

F = np.float32
WAVE_GROUPS = (32, 64, 128)      # launch_wave: the MatMulNBits blob with one of these group sizes and N % 4 == 0
NAIVE_SHARE = 0.01               # a condition on the inputs (measured 0.03 and more), not a tolerance on any result


# ----------------------------------------------------------------------------------------------- launch plans
def fused_shape(g):
    """`fused_shape` of csrc/rtn.hip: (rows per wave, waves per group) of the fused kernel, None for a group it does not hold."""
    for r in (16, 8, 4, 2, 1):
        if g % r == 0 and g // r <= 8:
            return r, g // r
    if g % 32 == 0 and g // 32 <= 8:
        return 32, g // 32
    return None


def wave_plan(k, n, g, bits):
    """`launch_wave` and the order-2 arm of `tile_of_block` (csrc/rtn.hip) restated: which build takes a [K, N] matrix of the
    MatMulNBits layout, its tiles, and for every block id the (row tile, column tile) it works on with the arms the map took."""
    assert g in WAVE_GROUPS and k % g == 0 and n % 4 == 0
    lpr = 1024 // g
    kgroups = k // g
    nstrips = -(-n // (4 * lpr))
    ncol_tiles = -(-nstrips // 4)
    nrow_tiles = kgroups
    gk = 4
    want_log2 = 9 if n % 16384 == 0 else (12 if n % 8192 == 0 else 10)
    tile_log2 = 6 + int(np.log2(lpr))
    xg_log2 = max(want_log2 - tile_log2, 0)
    small_idx = n * k * bits // 8 < (1 << 32)
    pair = small_idx and lpr == 8 and bits == 4 and kgroups % 2 == 0
    if pair:
        nrow_tiles = kgroups // 2
    build = "pair" if pair else (f"wave<{lpr},5>" if small_idx and lpr <= 16 else f"wave<{lpr}>")
    nblk = ncol_tiles * nrow_tiles
    assert nblk < (1 << 22)                                # beyond: order 0, which no case here reaches
    cw = 8 << xg_log2
    tiles, arms = [], set()
    for bid in range(nblk):
        b, r = divmod(bid, ncol_tiles * gk)
        gk_eff = min(gk, nrow_tiles - b * gk)
        arms.add("full_band" if gk_eff == gk else "short_band")
        cc, r = divmod(r, cw * gk_eff)
        w = min(cw, ncol_tiles - cc * cw)
        if w == cw:
            arms.add("full_chunk")
            within = r & (cw - 1)
            row_tile = b * gk + (r >> (3 + xg_log2))
            col_tile = cc * cw + ((within & 7) << xg_log2) + (within >> 3)
        else:
            arms.add("narrow_chunk")
            row_tile = b * gk + r // w
            col_tile = cc * cw + r % w
        tiles.append((row_tile, col_tile))
    tile_cols = 16 * lpr
    return {"build": build, "lpr": lpr, "ncol_tiles": ncol_tiles, "nrow_tiles": nrow_tiles, "gk": gk, "xg_log2": xg_log2,
            "tiles": tiles, "arms": frozenset(arms), "live_strips_of_last_tile": -(-(n - (ncol_tiles - 1) * tile_cols) // (4 * lpr))}


def build_of(k, n, g, bits, layout, emit_q=True):
    """The kernel `plan_route` gives a group-strategy call of these tests (16-byte aligned operands, ldw = N)."""
    if layout == "nbits" and g in WAVE_GROUPS and n % 4 == 0 and emit_q:
        return wave_plan(k, n, g, bits)["build"]
    rpw, _ = fused_shape(g)
    return f"fused<{rpw},{'vec4' if n % 4 == 0 else 'scalar'},{'q' if emit_q else 'params'}>"


def strip_lpr(g, layout, n):
    """Lanes per row piece of the build: a ballot of the fast path decides rows of 4 * LPR columns (the fused kernel: 256)."""
    return 1024 // g if layout == "nbits" and g in WAVE_GROUPS and n % 4 == 0 else 64


# ----------------------------------------------------------------------------------------------- inputs
def _levels(x, s, z, qmin, qmax, reciprocal):
    with np.errstate(all="ignore"):
        t = (x * (F(1) / s).astype(F)).astype(F) if reciprocal else (x / s).astype(F)
        return np.clip(np.rint(t).astype(np.int64) + z, qmin, qmax)


def _fast_paths(x, s, z, qmin, qmax):
    """The two fast paths of the kernels without their band, and where each meets an exact tie of its own arithmetic:
    the product form (fused kernel, `rtn_group_wave<32>`): k = rint(t), t = fl(x * fl(1/s)), residual fl(t - k);
    the fma form (five-wave and pair builds): u = rint(x * fl(1/s) + zp) in ONE rounding, residual fl(x * fl(1/s) + zp - u) --
    restated in float64, which holds the 48-bit product and the sum exactly.
    Returns (levels of the product form, levels of the fma form, |residual| >= 0.5 in either form)."""
    with np.errstate(all="ignore"):
        rinv = (F(1) / s).astype(F)
        t = (x * rinv).astype(F)
        k = np.rint(t)
        product = np.clip(k.astype(np.int64) + z, qmin, qmax)
        ex = x.astype(np.float64) * rinv.astype(np.float64) + z
        u = np.rint(ex)
        fma = np.clip(u.astype(np.int64), qmin, qmax)
        tie = (np.abs((t - k).astype(F)) >= F(0.5)) | (np.abs((ex - u).astype(F)) >= F(0.5))
        return product, fma, tie


def _at_boundary(b, d, s, zf, lo, hi):
    """fl((b + 0.5 - zp) * s) moved d ulp (|d| <= 2), clamped into the pinned range."""
    with np.errstate(all="ignore"):
        x = ((b.astype(F) + F(0.5) - zf).astype(F) * s).astype(F)
        for step in range(2):
            x = np.where(d > step, np.nextafter(x, F(np.inf)), x)
            x = np.where(d < -step, np.nextafter(x, F(-np.inf)), x)
        return np.clip(x, lo, hi).astype(F)


def boundary_dense(k, n, g, qtype, symmetric=False, reduce_range=False, clip_ratio=1.0, seed=0, huge=(), lpr=8):
    """fp32 [K, N] whose every element sits at a rounding boundary of its own (column, k-group).

    Two rows (they move with the column) of every (column, k-group) pin its range lo < 0 < hi: magnitude uniform(0.2, 3) * 2^e
    with e drawn per COLUMN from -12 .. 12 (the four columns of a lane have scales thousands of times apart), hi =
    uniform(0.2, 3) * -lo -- or -lo for a symmetric grid, where a one-sided range leaves half the levels unreachable.  The
    parameters of that range are the oracle's own (`min_max`, `qparams`): clipped and symmetric grids are the oracle's, not
    restated.  Every other row is fl((b + 0.5 - zp) * s) moved -2 .. +2 ulp and clamped into [lo, hi], with (b, ulp) uniform over
    the pairs of ALL boundaries of the grid, the two outside the clamp included, that are FREE: neither fast path of the kernels
    lands on an exact tie of its own arithmetic there (`_fast_paths`).  An exact tie has a residual of 0.5, which fires the
    redo whatever the band is; with one element in six on such a tie (what the unfiltered pairs give) every ballot fires on them
    and a band of any width passes.  Without them only `thr` stands between the fast path's integer and the result.
    Then every row of every strip of 4 * `lpr` columns that holds no element on which BOTH fast paths differ from rint(fl(x / s))
    gets one planted: a free pair of one of its columns on which they do.

    ``huge``: (k-group, column) pairs whose magnitude is 2^110: scale >= 1e30, `thr` = -1, the group is always redone."""
    assert k % g == 0
    r = np.random.default_rng([seed, k, n, g])
    kg = k // g
    qmin, qmax = O.qrange(qtype, symmetric, reduce_range)
    expo = np.exp2(r.integers(-12, 13, (1, 1, n)))
    big = np.zeros((kg, 1, n), bool)
    for kgi, col in huge:
        big[kgi, 0, col] = True
    unit = r.uniform(0.2, 3.0, (kg, 1, n))
    ratio = np.ones((kg, 1, n)) if symmetric else r.uniform(0.2, 3.0, (kg, 1, n))
    cb, cd = np.meshgrid(np.arange(qmin - 1, qmax + 1), np.arange(-2, 3), indexing="ij")
    pairs = cb.size
    for _ in range(50):
        mag = (unit * np.where(big, 2.0 ** 110, expo)).astype(F)
        lo = -mag
        hi = (ratio.astype(F) * mag).astype(F)
        pins = np.stack([lo.reshape(kg * n), hi.reshape(kg * n)], axis=1)
        s, z = O.qparams(*O.min_max(pins, "group", clip_ratio), qtype, symmetric, reduce_range)
        s = s.astype(F).reshape(kg, 1, n)
        z = z.astype(np.int64).reshape(kg, 1, n)
        zf = z.astype(F)
        # every (b, ulp) pair of every (column, k-group): which are free, and on which of those both fast paths differ from the division
        cand = _at_boundary(np.broadcast_to(cb.reshape(1, -1, 1), (kg, pairs, n)), np.broadcast_to(cd.reshape(1, -1, 1), (kg, pairs, n)), s, zf, lo, hi)
        product, fma, tie = _fast_paths(cand, s, z, qmin, qmax)
        exact = _levels(cand, s, z, qmin, qmax, False)
        free = ~tie
        cand_ok = free & (product != exact) & (fma != exact)
        barren = ~cand_ok.any(axis=1, keepdims=True)      # a range without one such pair (a scale whose reciprocal is exact, say): drawn again
        if not barren.any():
            break
        unit = np.where(barren, r.uniform(0.2, 3.0, (kg, 1, n)), unit)
        if not symmetric:
            ratio = np.where(barren, r.uniform(0.2, 3.0, (kg, 1, n)), ratio)
    assert free.any(axis=1).all() and not barren.any()
    # uniform over the free pairs: the free ones first (stable), then a uniform rank among them
    order = np.argsort(~free, axis=1, kind="stable")
    rank = np.floor(r.random((kg, g, n)) * free.sum(axis=1, keepdims=True)).astype(np.int64)
    x = np.take_along_axis(cand, np.take_along_axis(order, rank, axis=1), axis=1)
    # the pinning rows walk down the group from column to column, so no row of a strip (two columns at least) is all pins
    row_lo = (r.integers(0, g, (kg, 1, 1)) + 2 * np.arange(n).reshape(1, 1, n)) % g
    row_hi = (row_lo + 1) % g
    np.put_along_axis(x, row_lo, lo, axis=1)
    np.put_along_axis(x, row_hi, hi, axis=1)

    product, fma, _ = _fast_paths(x, s, z, qmin, qmax)
    exact = _levels(x, s, z, qmin, qmax, False)
    differs = (product != exact) & (fma != exact)
    pinned = np.zeros((kg, g, n), bool)
    np.put_along_axis(pinned, row_lo, True, axis=1)
    np.put_along_axis(pinned, row_hi, True, axis=1)
    width = 4 * lpr
    for c0 in range(0, n, width):
        c1 = min(c0 + width, n)
        for kgi, row in zip(*np.nonzero(~differs[:, :, c0:c1].any(axis=2))):
            cols = [c for c in range(c0, c1) if not pinned[kgi, row, c] and cand_ok[kgi, :, c].any()]
            if not cols:
                continue                               # the host test of the conditions sees it
            c = cols[r.integers(len(cols))]
            x[kgi, row, c] = cand[kgi, r.choice(np.nonzero(cand_ok[kgi, :, c])[0]), c]
    return np.ascontiguousarray(x.reshape(k, n))


def normal(k, n, seed=0):
    return np.random.default_rng([seed, k, n]).standard_normal((k, n), dtype=F)


def oracle(w, g, qtype, symmetric=False, reduce_range=False, clip_ratio=1.0):
    """(q [K, N], scale [N*K/g, 1], zp [N*K/g, 1]) of O.rtn_quantize, the strategy "group"."""
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return O.rtn_quantize(w, qtype, "group", g, symmetric, reduce_range, clip_ratio)


def conditions(w, g, qtype, symmetric=False, reduce_range=False, clip_ratio=1.0, lpr=8):
    """What makes ``w`` a test of the fast path's band and its redo, from NumPy and the oracle alone:
    naive_share     share of elements where clip(rint(fl(x * fl(1/s))) + zp) is not the oracle's integer;
    fma_share       the same for the one-rounding form rint(x * fl(1/s) + zp) of the five-wave and pair builds;
    exact_ties      share of elements on which either form has a residual of 0.5 or more (`_fast_paths`): they fire the redo
                    whatever the band is, so there must be none;
    least_level     (level, count) of the least used level among those an input of these ranges can reach -- the whole grid,
                    but for level 0 of the symmetric unsigned grids (zero = 8, 7 levels either side: nothing rounds below 1);
    strip_rows      share of the rows of strips of 4 * lpr columns that hold at least one element on which BOTH forms differ."""
    k, n = w.shape
    q, s, z = oracle(w, g, qtype, symmetric, reduce_range, clip_ratio)
    kg = k // g
    qmin, qmax = O.qrange(qtype, symmetric, reduce_range)
    S = s.reshape(n, kg).T[:, None, :]
    Z = z.reshape(n, kg).T[:, None, :].astype(np.int64)
    product, fma, tie = _fast_paths(w.reshape(kg, g, n), S, Z, qmin, qmax)
    want = q.astype(np.int64)
    d_product, d_fma = product.reshape(k, n) != want, fma.reshape(k, n) != want
    both = d_product & d_fma
    first = qmin + 1 if symmetric and qmin == 0 and not reduce_range else qmin
    counts = np.bincount((want - qmin).reshape(-1), minlength=qmax - qmin + 1)[first - qmin:]
    width = 4 * lpr
    strips = [both[:, c0:c0 + width].any(axis=1) for c0 in range(0, n, width)]
    return {"naive_share": float(d_product.mean()), "fma_share": float(d_fma.mean()), "exact_ties": float(tie.mean()),
            "least_level": (int(first + counts.argmin()), int(counts.min())), "strip_rows": float(np.mean(strips)),
            "levels": int(qmax - first + 1)}


# ----------------------------------------------------------------------------------------------- layouts and reports
def blob_to_kn(blob, k, n, g, bits):
    """MatMulNBits blob [N, K/g, g*bits/8] -> the unsigned levels [K, N] (qrules/_common.py:72-87: even k in the low nibble)."""
    b = np.asarray(blob, dtype=np.uint8).reshape(n, k // g, g * bits // 8)
    if bits == 4:
        u = np.empty((n, k // g, g), np.uint8)
        u[:, :, 0::2] = b & 0x0F
        u[:, :, 1::2] = b >> 4
    else:
        u = b
    return np.ascontiguousarray(u.reshape(n, k).T)


def packed4_to_kn(packed, k, n):
    """[K, N/2] nibble pairs (core/_pack.py:8-22: column 2j in the low nibble of byte j) -> the unsigned nibbles [K, N]."""
    p = np.asarray(packed, dtype=np.uint8).reshape(k, n // 2)
    u = np.empty((k, n), np.uint8)
    u[:, 0::2] = p & 0x0F
    u[:, 1::2] = p >> 4
    return u


def unsigned_levels(q, bits):
    """The oracle's [K, N] integers as the bytes / nibbles a layout stores (two's complement)."""
    return (np.asarray(q).astype(np.int16) & ((1 << bits) - 1)).astype(np.uint8)


def where_wrong(got, want, k, n, g, lpr=8):
    """Where two [K, N] integer matrices differ, in the kernels' terms: the count, the (k-group, column tile, strip) cells and the
    lane sets (16 rows of a group each) that hold most of it, and the first element with both values.  '' when they are equal."""
    got, want = np.asarray(got).reshape(k, n), np.asarray(want).reshape(k, n)
    bad = got != want
    if not bad.any():
        return ""
    rows, cols = np.nonzero(bad)
    strip, tile = 4 * lpr, 16 * lpr
    cells: dict = {}
    sets: dict = {}
    for rr, cc in zip(rows.tolist(), cols.tolist()):
        key = (rr // g, cc // tile, (cc % tile) // strip)
        cells[key] = cells.get(key, 0) + 1
        sets[(rr % g) // 16] = sets.get((rr % g) // 16, 0) + 1
    top = sorted(cells.items(), key=lambda kv: -kv[1])[:6]
    r0, c0 = int(rows[0]), int(cols[0])
    return (f"{int(bad.sum())} of {k * n} elements differ in {len(cells)} (k-group, column tile, strip) cells; most: "
            + ", ".join(f"{key}: {cnt}" for key, cnt in top)
            + "; per lane set: " + ", ".join(f"{h}: {cnt}" for h, cnt in sorted(sets.items()))
            + f"; first at row {r0} (k-group {r0 // g}, row {r0 % g} of it), column {c0} (lane column {(c0 % strip) // 4}, slot {c0 % 4}): "
            + f"got {int(got[r0, c0])}, oracle {int(want[r0, c0])}")


def where_params_wrong(got, want, n, kgroups, what):
    got, want = np.asarray(got).reshape(n, kgroups), np.asarray(want).reshape(n, kgroups)
    bad = got.view(np.uint32 if got.dtype == np.float32 else got.dtype) != want.view(np.uint32 if want.dtype == np.float32 else want.dtype)
    if not bad.any():
        return ""
    cols, kgs = np.nonzero(bad)
    c0, k0 = int(cols[0]), int(kgs[0])
    return (f"{what}: {int(bad.sum())} of {n * kgroups} entries differ, k-groups {sorted(set(kgs.tolist()))[:8]}, columns {sorted(set(cols.tolist()))[:8]} ...; "
            f"first at column {c0}, k-group {k0}: got {got[c0, k0]!r}, oracle {want[c0, k0]!r}")


# ----------------------------------------------------------------------------------------------- the cases of the GPU file
@dataclass(frozen=True)
class Case:
    id: str
    k: int
    n: int
    g: int
    qtype: str
    layout: str = "nbits"
    build: str = ""              # the build the case is there for (checked on the host against `build_of`)
    symmetric: bool = False
    reduce_range: bool = False
    clip_ratio: float = 1.0
    huge: tuple = ()
    emit_q: bool = True
    seed: int = 0

    @property
    def bits(self):
        return O.BITWIDTH[self.qtype]

    @property
    def lpr(self):
        return strip_lpr(self.g, self.layout, self.n)

    @property
    def grid(self):
        return self.qtype, self.symmetric, self.reduce_range, self.clip_ratio


def _grids(prefix, k, n, g, qtype, layout, build):
    """asymmetric / symmetric / reduce_range x clip_ratio 1.0 / 0.9 on one build (the plain asymmetric case is in the list already)."""
    out = []
    for sym, rr, clip in ((False, False, 0.9), (True, False, 1.0), (True, False, 0.9), (False, True, 1.0), (False, True, 0.9)):
        name = f"{prefix}-{'sym' if sym else 'rr'}" if sym or rr else f"{prefix}-asym"
        out.append(Case(f"{name}-clip{clip}", k, n, g, qtype, layout, build, sym, rr, clip))
    return out


# Section 1: two column tiles, two or three k-groups of every build.
BOUNDARY = [
    Case("pair-uint4", 256, 256, 128, "uint4", build="pair"),
    Case("pair-int4", 256, 256, 128, "int4", build="pair"),
    *_grids("pair-uint4", 256, 256, 128, "uint4", "nbits", "pair"),
    Case("pair-uint4-huge", 256, 256, 128, "uint4", build="pair", huge=((0, 5), (1, 6), (0, 130), (1, 255)), seed=1),
    Case("wave8x5-uint4", 384, 256, 128, "uint4", build="wave<8,5>"),          # K / g = 3, odd: the four-wave build
    Case("wave8x5-int4", 384, 256, 128, "int4", build="wave<8,5>"),
    Case("wave8x5-int8", 384, 256, 128, "int8", build="wave<8,5>"),
    Case("wave8x5-uint8", 256, 256, 128, "uint8", build="wave<8,5>"),          # 8-bit: never the pair build
    Case("wave16x5-uint4", 192, 512, 64, "uint4", build="wave<16,5>"),
    Case("wave16x5-int8", 128, 512, 64, "int8", build="wave<16,5>"),
    Case("wave32-uint4", 96, 1024, 32, "uint4", build="wave<32>"),
    Case("wave32-uint8", 64, 1024, 32, "uint8", build="wave<32>"),
    *[Case(f"fused-kn-g{g}", 2 * g, 512, g, "uint4", "kn", f"fused<{fused_shape(g)[0]},vec4,q>") for g in (16, 32, 64, 128, 256)],
    Case("fused-kn-g128-int8", 384, 512, 128, "int8", "kn", "fused<16,vec4,q>"),
    *_grids("fused-kn-g128-int8", 384, 512, 128, "int8", "kn", "fused<16,vec4,q>"),
    *[Case(f"fused-packed4-g{g}", 2 * g, 512, g, "int4", "kn_packed4", f"fused<{fused_shape(g)[0]},vec4,q>") for g in (16, 32, 64, 128, 256)],
    Case("fused-packed4-g128-n516", 256, 516, 128, "uint4", "kn_packed4", "fused<16,vec4,q>"),   # N % 8 == 4: the two-byte stores
    Case("fused-kn-scalar-n258", 96, 258, 32, "uint8", "kn", "fused<16,scalar,q>"),              # N % 4 != 0: lane-strided columns
    Case("fused-params-g64", 192, 512, 64, "uint4", "kn", "fused<16,vec4,params>", emit_q=False),
    Case("fused-params-g128-int8-sym", 256, 512, 128, "int8", "kn", "fused<16,vec4,params>", symmetric=True, emit_q=False),
    Case("fused-blob-g16", 48, 512, 16, "uint4", "nbits", "fused<16,vec4,q>"),
    Case("fused-blob-g256-int4", 512, 512, 256, "int4", "nbits", "fused<32,vec4,q>"),
]
BOUNDARY_BY_ID = {c.id: c for c in BOUNDARY}

# ... through the list and the batched entry points (two matrices each; the second one's seed differs)
LISTS = [("pair-uint4", "many"), ("pair-int4", "batched"), ("wave16x5-uint4", "many"), ("wave16x5-int8", "batched")]

# Section 4: right edges of the pair build, K = 256: one lane column; a strip and one lane column; three strips and one lane column;
# four strips less one lane column; a tile of one lane column behind a full tile.
EDGES = [Case(f"pair-edge-n{n}", 256, n, 128, "uint4", build="pair", seed=4) for n in (4, 36, 100, 124, 132)]

# Section 2: block orders (i.i.d. normal weights): (k, n, g, build, xg_log2, arms of the map, live strips of the last column tile)
ALL_ARMS = frozenset({"full_band", "short_band", "full_chunk", "narrow_chunk"})
ORDERS = [
    (1280, 2180, 128, "pair", 1, ALL_ARMS, 1),                                           # 16 tiles + 2, five row tiles
    (1280, 8192, 128, "pair", 3, frozenset({"full_band", "short_band", "full_chunk"}), 4),   # one chunk of 64
    (1280, 16384, 128, "pair", 0, frozenset({"full_band", "short_band", "full_chunk"}), 4),
    (1536, 2048, 128, "pair", 1, frozenset({"full_band", "short_band", "full_chunk"}), 4),   # six row tiles: 4 + 2
    (384, 2304, 64, "wave<16,5>", 0, ALL_ARMS, 4),                                       # nine tiles of 256: 8 + 1; six row tiles
    (384, 8192, 64, "wave<16,5>", 2, frozenset({"full_band", "short_band", "full_chunk"}), 4),
]

# Section 3: store arms of the pair build: (scale offset in bytes from an 8-byte aligned address, zero-point offset)
STORE_SHAPES = [(256, 128), (512, 132)]
STORE_OFFSETS = [(0, 0), (4, 0), (0, 1), (4, 1)]
TABLE_OFFSETS = [(0, 0), (4, 1), (0, 3)]


@functools.lru_cache(maxsize=None)
def boundary_input(case_id, seed_shift=0):
    """(w, (q, scale, zp) of the oracle) of a boundary-dense case; computed once, shared, read-only."""
    c = {**BOUNDARY_BY_ID, **{e.id: e for e in EDGES}}[case_id]
    w = boundary_dense(c.k, c.n, c.g, c.qtype, c.symmetric, c.reduce_range, c.clip_ratio, c.seed + seed_shift, c.huge, c.lpr)
    ref = oracle(w, c.g, *c.grid)
    for a in (w, *ref):
        a.setflags(write=False)
    return w, ref


@functools.lru_cache(maxsize=None)
def boundary_conditions(case_id):
    c = {**BOUNDARY_BY_ID, **{e.id: e for e in EDGES}}[case_id]
    return conditions(boundary_input(case_id)[0], c.g, *c.grid, lpr=c.lpr)


@functools.lru_cache(maxsize=None)
def normal_input(k, n, g, qtype="uint4", seed=0):
    w = normal(k, n, seed)
    ref = oracle(w, g, qtype)
    for a in (w, *ref):
        a.setflags(write=False)
    return w, ref
