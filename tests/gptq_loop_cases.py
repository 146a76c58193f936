"""What the exact tests of the GPTQ corrected-mode row loop share (test_gptq_loop_cases.py, test_gptq_loop_exact_gpu.py): plain numpy
and the oracle, no library call.

`restate`    the reference loop (gptq.py:153-216 with the corrected indexing, as `oq_oracle.gptq(mode="corrected")` walks it) on a GIVEN
             upper factor U and GIVEN initial parameters, in float64 -- or, with dtype = np.float32, with every step rounded to fp32;
`exact_ok`   the conditions under which `oq_gptq_loop_f32` owes the float64 loop's bytes, whatever its blocking and GEMM route;
recipes      seeded integer data that satisfies them (`exact_case`), and the random fp32 family (`fp32_case`);
`contraction_case`  data on which a fused multiply-add in the row update moves integers;
`routes`     the host's dispatch of csrc/gptq_loop.hip restated: which kernel walks which rows, which update leg follows;
`locate`     wrong outputs -> launch ordinal, kernel, slab, lane of the 16 and column of the wave; `describe` as text.

Why the loop can be exact.  Take a column c with the unit u_c = s_c 2^-6, s_c a power of two.  Weights are multiples of u_c; the scale of
every group is s_c (or 2 s_c), so w / s has at most 24 bits, the dequantized value is a multiple of s_c and the residual w - q one of
u_c.  The diagonal of U is 1, 1/2 or 1/4, so the error (w - q) / d is again a multiple of u_c, and the off-diagonal entries of U are
small integers, so every product U[i][j] e_i and every partial sum of them is one.  A multiple of u_c below 2^24 u_c is an fp32 number:
with `mass` = |w0| + sum_i |U[i][j]| |e_i| < 2^24 u_c nothing is ever rounded, in whatever order the kernels, the panel update, the fp32
GEMM or the fp16-piece GEMM add.  The group parameters come out of (max - min) / (qmax - qmin) = s_c exactly because two anchor rows
per group hold the ends of the grid, (qmin - z) s and (qmax - z) s, and nothing reaches them (their columns of U are zero).
"""
import collections
import functools
import math
import zlib

import numpy as np

import oq_oracle as O
import piece_gemm_cases as P

LOOP_ROWS = 128                 # kLoopMaxRows: rows of one launch
SUPER_ROWS = 512                # kSuperRows
PANEL_TILE = 64                 # kPanelTile
FRAC = 64                       # weights are multiples of s / FRAC


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------ the reference loop on a given U
Restated = collections.namedtuple("Restated", "q q_deq used_scale used_zp w err exact mass_units")


def restate(w, u, qtype, group_size, block_size, symmetric, reduce_range, init_scale, init_zp, dtype=np.float64, unit=None):
    """-> Restated.  q [K, N] int64 levels, q_deq [K, N], used_scale / used_zp [ceil(K / g), N] (None without loop groups), the final
    W, err: the per-block Err as a list of (i1, [rows, N]); all of `dtype`.  The group parameters of gptq.py:168-184 come through
    `O.min_max` / `O.qparams` on the fp32 rows of W -- the matrix the block products update (gptq.py:208), not the block's copy W1.

    dtype = np.float64: `exact` says whether every quotient, product and difference was its own fp32 rounding, and with `unit` [N]
    `mass_units` is max over elements of (|w0| + sum_i |U[i][j]| |e_i|) / unit.  dtype = np.float32: every step is rounded as the
    kernels round it (IEEE divide, rint, one rounding for the product, one for the subtraction); the product behind a block is
    numpy's fp32 matmul, which the kernels owe bit for bit only where it adds exact zeros."""
    K, N = w.shape
    g = int(group_size) if group_size and group_size > 0 else 0
    qmin, qmax = O.qrange(qtype, symmetric, reduce_range)
    W = np.array(w, dtype=dtype)
    U = np.asarray(u, dtype=dtype)
    s = np.broadcast_to(np.asarray(init_scale, dtype=np.float32).reshape(-1), (N,)).astype(dtype)
    z = np.broadcast_to(np.asarray(init_zp).reshape(-1), (N,)).astype(np.int64)
    q = np.zeros((K, N), dtype=np.int64)
    qd = np.zeros((K, N), dtype=dtype)
    used_s = np.zeros((ceil_div(K, g), N), dtype=dtype) if g else None
    used_z = np.zeros((ceil_div(K, g), N), dtype=np.int64) if g else None
    errs, exact = [], True
    mass = np.abs(np.asarray(w, dtype=np.float64))
    absu = np.abs(np.asarray(u, dtype=np.float64))

    def is32(x):
        return bool(np.array_equal(x, x.astype(np.float32).astype(x.dtype)))

    with np.errstate(all="ignore"):
        for i1 in range(0, K, block_size):
            i2 = min(i1 + block_size, K)
            W1 = W[i1:i2].copy()
            E1 = np.zeros_like(W1)
            for i in range(i2 - i1):
                row = W1[i].copy()
                d = U[i1 + i, i1 + i]
                if g and (i1 + i) % g == 0:
                    rows32 = W[i1 + i:i1 + i + g].astype(np.float32)
                    lo, hi = O.min_max(rows32.T, "channel")
                    ps, pz = O.qparams(lo, hi, qtype, symmetric, reduce_range)
                    s, z = ps.reshape(-1).astype(dtype), pz.reshape(-1).astype(np.int64)
                    used_s[(i1 + i) // g], used_z[(i1 + i) // g] = s, z
                y = row / s
                level = O.quantize(row, s, z, qtype, symmetric, reduce_range).astype(np.int64)
                deq = O.dequantize(level, s, z).astype(dtype)
                t = row - deq
                e = t / d
                prod = np.outer(U[i1 + i, i1 + i:i2], e)
                new = W1[i:] - prod
                if dtype == np.float64:
                    exact = exact and is32(y) and is32(deq) and is32(t) and is32(e) and is32(prod) and is32(new)
                W1[i:] = new
                q[i1 + i], qd[i1 + i], E1[i] = level, deq, e
            errs.append((i1, E1))
            if i2 < K:
                tail = U[i1:i2, i2:].T @ E1
                new = W[i2:] - tail
                if dtype == np.float64:
                    exact = exact and is32(tail) and is32(new)
                W[i2:] = new
            mass += absu[i1:i2].T @ np.abs(E1.astype(np.float64))
    mass_units = float((mass / np.asarray(unit, dtype=np.float64)[None, :]).max()) if unit is not None else None
    return Restated(q, qd, used_s, used_z, W, errs, exact, mass_units)


# ------------------------------------------------------------------------------------ the host's dispatch, restated
def _lcm(a, b):
    return a // math.gcd(a, b) * b


def super_rows(block_size, g):
    """S of oq_gptq_loop_f32: the rows whose product behind them is deferred to one GEMM."""
    if block_size > LOOP_ROWS:
        return block_size
    unit = _lcm(block_size, g) if g > 0 else block_size
    return SUPER_ROWS // unit * unit if unit <= SUPER_ROWS else block_size


def routes(K, N, g, block_size, mode="corrected", method=None):
    """-> dict(S, tall, launches, deferred).  A launch: dict(ord, i1, count, kernel 'rows16' | 'block', slabs: 'live0' .. 'live7' |
    'ragged' per 16-row slab of a rows16 launch, block_start, super_start, update: None | ('panel', ()) | ('gemm_tn', reasons)).
    A deferred product: dict(s0, s_end, M, Kd, leg 'pieces' | 'gemm_tn').  Operand bases are taken 16-byte aligned, as torch's are."""
    g = g if g and g > 0 else 0
    tall = block_size > LOOP_ROWS
    sub = LOOP_ROWS if tall else block_size
    S = super_rows(block_size, g)
    rows16 = mode == "corrected" and (g == 0 or g % 16 == 0) and sub % 16 == 0
    per_block = ceil_div(block_size, LOOP_ROWS) if tall else 1
    launches, deferred = [], []
    for s0 in range(0, K, S):
        s_end = min(s0 + S, K)
        for i1 in range(s0, s_end, sub):
            count = min(s_end - i1, sub)
            i2 = i1 + count
            la = dict(ord=(i1 // block_size) * per_block + (i1 % block_size) // LOOP_ROWS, i1=i1, count=count,
                      kernel="rows16" if rows16 and i1 % 16 == 0 else "block", block_start=i1 % block_size == 0, super_start=i1 == s0,
                      slabs=[], update=None)
            if la["kernel"] == "rows16":
                nslabs = ceil_div(count, 16)
                la["slabs"] = ["ragged" if count - 16 * k0 < 16 else f"live{nslabs - 1 - k0}" for k0 in range(nslabs)]
            if i2 < s_end:
                M = s_end - i2
                why = []
                if M % 4 or M < 4:
                    why.append("M % 4")
                if N % 4 or N < 4:
                    why.append("N % 4")                               # also ldb = N
                if K % 4:
                    why.append("lda % 4")
                if (i1 * K + i2) % 4:
                    why.append("A unaligned")
                la["update"] = ("gemm_tn", tuple(why)) if why else ("panel", ())
            launches.append(la)
        if s_end < K:
            M, Kd = K - s_end, s_end - s0
            deferred.append(dict(s0=s0, s_end=s_end, M=M, Kd=Kd, leg="pieces" if method != "f32" and Kd >= 64 and M * N >= 1 << 20 else "gemm_tn"))
    return dict(S=S, tall=tall, launches=launches, deferred=deferred)


# ------------------------------------------------------------------------------------ the exact recipes
Case = collections.namedtuple("Case", "name w u qtype g block_size symmetric reduce_range init_scale init_zp scale zp unit planted anchors "
                                      "clamps versions")
ZP_BASE = {"int8": -1, "int4": -1, "uint8": 100, "uint4": 5}        # + c % 3: zero points of both parities, never 0 for unsigned
PER_COLUMN = {8: 12, 4: 5}                                         # sources per column outside a dense block
MARGIN = {8: 48, 4: 5}                                             # levels a planted weight keeps from either end of the grid


def _rng(name):
    return np.random.default_rng([zlib.crc32(name.encode()), 37])


def exact_case(name, K, N, qtype, g, block_size, dense=False, symmetric=False, reduce_range=False, init_count=None, versions=()):
    """Seeded data on which the loop is exact (module docstring).
    dense: every U[i][j], i < j, inside a 128-row launch is +-1 (8-bit types only) instead of PER_COLUMN sources per column.
    versions: parameter-version probes (source group, target group): a clamp row in the source group with e = -(qmax - qmin) s whose
    only coefficient is 1 on the maximum anchor of the target group -- that group's scale is s if its rows are read before the
    update reaches W and 2 s after."""
    r = _rng(name)
    g = g if g and g > 0 else 0
    bits = O.BITWIDTH[qtype]
    qmin, qmax = O.qrange(qtype, symmetric, reduce_range)
    cols = np.arange(N)
    s = np.ldexp(1.0, cols % 3 - 1)
    if symmetric:
        zero = int(np.round((qmax + qmin) / 2.0))
        z = np.full(N, zero, dtype=np.int64)
    else:
        z = np.clip(ZP_BASE[qtype] + cols % 3, qmin + 1, qmax - 1).astype(np.int64)
    unit = s / FRAC
    sub = LOOP_ROWS if block_size > LOOP_ROWS else block_size
    launch_of = np.arange(K) // block_size * 64 + np.arange(K) % block_size // LOOP_ROWS        # an id per launch
    super_of = np.arange(K) // super_rows(block_size, g)

    # anchors: two rows per group, the same for all columns; which one holds the minimum alternates by column
    anchors = np.zeros(K, dtype=bool)
    ngroups = ceil_div(K, g) if g else 0
    lo_row, hi_row = {}, {}
    for G in range(ngroups):
        start, glen = G * g, min(g, K - G * g)
        assert glen >= 2, "a group needs two anchor rows"
        o0 = (3 * G + 1) % glen
        o1 = (o0 + 1 + (5 * G) % (glen - 1)) % glen
        lo_row[G], hi_row[G] = start + min(o0, o1), start + max(o0, o1)      # hi after lo: a version probe's source can precede it
        anchors[[start + o0, start + o1]] = True
    target_groups = {t for _, t in versions}

    # clamp rows (two or one level outside the grid, large exact errors): only without loop groups, where no range is read from W.
    # Version probes are ordinary rows that nothing reaches: w = s / 4 (level z, residual s / 4 under the scale s and under 2 s),
    # d = 1 / 4, so e = s exactly, and the one coefficient -(qmax - qmin) on the target's maximum anchor moves it up by the grid's span.
    clamps = np.zeros(K, dtype=bool)
    free = np.flatnonzero(~anchors)
    ordinary = r.choice(free, size=min(3, len(free) // 6), replace=False) if not g and len(free) >= 6 else np.array([], dtype=np.int64)
    probes, factor = {}, {}
    for src, tgt in versions:
        lo_s, hi_s = src * g, min(src * g + g, K)
        limit = hi_row[tgt] if src == tgt else hi_s
        cand = [i for i in range(lo_s, limit) if not anchors[i] and i not in probes]
        i = cand[len(cand) // 2]
        probes[i] = tgt
        assert tgt not in factor, "one probe per target group"
        factor[tgt] = 1 if i // block_size >= (tgt * g) // block_size else 2      # the reference reads W as the group's block found it
    clamps[ordinary] = True
    is_probe = np.zeros(K, dtype=bool)
    is_probe[list(probes)] = True

    # U
    u = np.zeros((K, K), dtype=np.float64)
    diag = r.choice([1.0, 0.5, 0.25], size=K, p=[0.5, 0.3, 0.2] if bits == 8 else [0.8, 0.2, 0.0])
    diag[anchors | clamps] = 1.0
    diag[is_probe] = 0.25
    sources_ok = ~anchors & ~clamps & ~is_probe     # anchors have e = 0 and must send nothing when a probe has moved them
    targets_ok = ~anchors & ~clamps & ~is_probe
    for j in np.flatnonzero(targets_ok):
        cand = np.flatnonzero(sources_ok[:j])
        if not len(cand):
            continue
        if dense:
            pick = cand[launch_of[cand] == launch_of[j]]
        else:
            # a third from the row's own launch, a third from its super-block, the rest from anywhere above
            n = PER_COLUMN[bits]
            pools = [cand[launch_of[cand] == launch_of[j]], cand[(super_of[cand] == super_of[j]) & (launch_of[cand] != launch_of[j])], cand]
            pick = np.unique(np.concatenate([r.choice(p, size=min(len(p), ceil_div(n, 3)), replace=False) for p in pools if len(p)]))
        u[pick, j] = r.choice([-1.0, 1.0, 2.0, -2.0], size=len(pick), p=[0.5, 0.5, 0, 0] if dense or bits == 4 else [0.45, 0.45, 0.05, 0.05])
    for i in ordinary:                              # two targets each
        cand = np.flatnonzero(targets_ok[i + 1:]) + i + 1
        if len(cand):
            u[i, r.choice(cand, size=min(2, len(cand)), replace=False)] = r.choice([-1.0, 1.0], size=min(2, len(cand)))
    for i, tgt in probes.items():
        u[i, :] = 0.0
        u[i, hi_row[tgt]] = -float(qmax - qmin)
    u[np.arange(K), np.arange(K)] = diag

    # W: levels well inside the grid, fractions in 64ths with ties at the half
    margin = MARGIN[bits] if qmax - qmin > 2 * MARGIN[bits] + 2 else max(1, (qmax - qmin) // 2 - 1)
    level = r.integers(qmin + margin, qmax - margin + 1, size=(K, N))
    frac = r.integers(-FRAC // 2, FRAC // 2 + 1, size=(K, N))
    tie = r.random((K, N)) < 0.25
    frac[tie] = r.choice([-FRAC // 2, FRAC // 2], size=int(tie.sum()))
    w = (level - z[None, :] + frac / FRAC) * s[None, :]
    out = 1 if bits == 4 else 2
    for n, i in enumerate(ordinary):
        high = (cols + n) % 2 == 0
        w[i] = np.where(high, qmax - z + out + 0.25, qmin - z - out - 0.5) * s
    for i in probes:
        w[i] = 0.25 * s
    planted = None
    if g:
        planted = np.tile(s, (ngroups, 1))
        for tgt, f in factor.items():
            planted[tgt] *= f
        for G in range(ngroups):
            alt = (cols + G) % 2 == 0 if G not in target_groups else np.zeros(N, dtype=bool)      # a probe's target holds the maximum in every column
            lo_v, hi_v = (qmin - z) * s, (qmax - z) * s
            w[lo_row[G]] = np.where(alt, hi_v, lo_v)
            w[hi_row[G]] = np.where(alt, lo_v, hi_v)
    init_count = N if init_count is None else init_count
    if init_count == 1:
        assert not g, "one initial parameter for all columns: no loop groups, one scale"
        s = np.full(N, 1.0)
        z = np.full(N, z[0])
        unit = s / FRAC
        w = (level - z[None, :] + frac / FRAC)
        for n, i in enumerate(ordinary):
            w[i] = np.where((cols + n) % 2 == 0, qmax - z + out + 0.25, qmin - z - out - 0.5)
    w32, u32 = w.astype(np.float32), u.astype(np.float32)
    assert np.array_equal(w32, w) and np.array_equal(u32, u)
    return Case(name, w32, u32, qtype, g, block_size, symmetric, reduce_range, s[:init_count].astype(np.float32), z[:init_count].astype(np.int32),
                s, z, unit, planted, anchors, clamps, tuple((i, t) for i, t in probes.items()))


def piece_legs(case):
    return [d for d in routes(*case.w.shape, case.g, case.block_size)["deferred"] if d["leg"] == "pieces"]


@functools.lru_cache(maxsize=None)
def restated(name):
    c = CASES[name]()
    return c, restate(c.w, c.u, c.qtype, c.g, c.block_size, c.symmetric, c.reduce_range, c.init_scale, c.init_zp, unit=c.unit)


def exact_ok(case, res=None):
    """Every quotient, product and difference of the float64 loop is its own fp32 rounding, every element's absolute mass stays below
    2^24 units, and where the host sends a deferred product to the fp16-piece GEMM that product is exact there too."""
    if res is None:
        res = restate(case.w, case.u, case.qtype, case.g, case.block_size, case.symmetric, case.reduce_range, case.init_scale, case.init_zp,
                      unit=case.unit)
    ok = res.exact and res.mass_units < 2.0 ** 24
    S = super_rows(case.block_size, case.g)
    for leg in piece_legs(case):
        s0, s_end = leg["s0"], leg["s_end"]
        if case.block_size > LOOP_ROWS:
            err = dict(res.err)[s0]
        else:
            err = np.concatenate([e for i1, e in res.err if s0 <= i1 < s_end])
        assert err.shape[0] == s_end - s0 and s_end - s0 <= max(S, case.block_size)
        ok = ok and P.exact_ok(case.u[s0:s_end, s_end:].T.copy(), err.astype(np.float32), False)
    return bool(ok)


# ------------------------------------------------------------------------------------ the case list
ONE_LAUNCH_K = (1, 15, 16, 17, 100, 127, 128)
ONE_LAUNCH_N = (1, 3, 4, 5, 16, 17, 63, 64, 65, 130)
WIDE_N = (4100, 12292)          # at K = 32: the rows16 workgroup takes 8 and 16 waves
#                K, block_size, g, N
MULTI_LAUNCH = [(256, 128, 128, 64), (384, 128, 64, 52), (200, 64, 16, 130), (640, 128, 48, 132), (1100, 128, 256, 64), (700, 128, 1024, 52),
                (640, 320, 64, 130), (600, 256, 128, 132), (520, 24, 0, 64), (300, 128, 24, 52), (260, 18, 0, 132), (130, 64, 64, 64),
                (130, 64, 0, 130),
                (520, 22, 0, 64), (134, 17, 0, 64)]        # the panel update's fallback for one reason at a time: M % 4 | A unaligned, lda % 4
TYPES = ("int4", "uint4", "int8", "uint8")


def _cases():
    c = {}

    def add(name, K, N, qtype, g, block_size, **k):
        c[name] = functools.partial(exact_case, name, K, N, qtype, g, block_size, **k)
        SHAPES[name] = (K, N, g, block_size)

    for i, K in enumerate(ONE_LAUNCH_K):                                  # every K at two widths, every N at two heights
        for N in (ONE_LAUNCH_N[i], ONE_LAUNCH_N[(i + 5) % 10], ONE_LAUNCH_N[(2 * i + 3) % 10]):
            add(f"one-{K}x{N}", K, N, "int8", 0, 128, dense=True, init_count=N if (K + N) % 2 else 1)
    add("one-128x64-groups", 128, 64, "uint8", 32, 128, dense=True)
    add("one-100x17-groups", 100, 17, "int8", 16, 128, dense=True)
    for N in WIDE_N:
        add(f"wide-32x{N}", 32, N, "int8", 16, 128, dense=True)
    for K, bs, g, N in MULTI_LAUNCH:
        add(f"multi-{K}-{bs}-{g}-{N}", K, N, "uint8" if (K + N) % 3 == 0 else "int8", g, bs)
    add("deferred-1536x1024", 1536, 1024, "int8", 128, 128)
    for t in TYPES:                                                      # types and grids; the 4-bit ones also in the packed layout
        add(f"type-{t}", 256, 20, t, 32 if t != "uint4" else 64, 128 if t != "uint4" else 32)
    add("type-int4-n6", 200, 6, "int4", 40, 64)                          # N % 4 = 2; g % 16 != 0: packed on the block kernel under both modes
    add("type-uint4-n130", 144, 130, "uint4", 48, 128)
    add("type-int8-symmetric", 256, 20, "int8", 64, 128, symmetric=True)
    add("type-uint8-reduced", 256, 20, "uint8", 32, 128, reduce_range=True)
    add("type-int8-reduced", 160, 12, "int8", 32, 64, reduce_range=True)
    # parameter versions: (source group, target group)
    add("versions-1100-128-128", 1100, 20, "int8", 128, 128, versions=((1, 1), (1, 2), (2, 5), (0, 8)))       # same block | super-block | behind it
    add("versions-640-128-64", 640, 20, "uint8", 64, 128, versions=((0, 0), (0, 1), (1, 2), (3, 9)))          # (0, 1): same block, later group
    add("versions-600-256-128", 600, 20, "int8", 128, 256, versions=((0, 0), (0, 1), (1, 2), (2, 4)))         # tall: (0, 1) same block, other launch
    add("versions-300-128-24", 300, 20, "int8", 24, 128, versions=((0, 1), (4, 6), (2, 11)))                  # block kernel under both modes
    # lcm(128, 48) = 384: group 10 (rows 480 .. 527) starts in the second super-block and its maximum anchor lies past row 512
    add("versions-640-128-48", 640, 20, "int8", 48, 128, versions=((0, 0), (2, 5), (1, 10)))
    return c


SHAPES = {}                     # name -> (K, N, g, block_size)
CASES = _cases()
VERSION_CASES = [n for n in CASES if n.startswith("versions-")]
PACKED_CASES = ["type-int4", "type-uint4", "type-int4-n6", "type-uint4-n130"]


def expected_versions(case):
    """For each probe's target group: 1 where the reference reads the group's rows before the probe's error reaches W (the probe sits
    in the block the group starts in, or later), else 2 -- the factor on the column's scale."""
    return {tgt: 1 if i // case.block_size >= (tgt * case.g) // case.block_size else 2 for i, tgt in case.versions}


# ------------------------------------------------------------------------------------ the fp32 family
def fp32_case(K, N, g, block_size, seed=0):
    """Random float weights; U with random floats inside each launch's own diagonal block and zeros elsewhere, so every update product
    adds exact zeros and the kernels owe `restate(dtype=np.float32)` bit for bit.  -> (w, u, init_scale, init_zp), uint8."""
    r = np.random.default_rng([K, N, g, block_size, seed])
    w = (r.standard_normal((K, N)) * np.exp(r.uniform(-2, 2, size=(1, N)))).astype(np.float32)
    u = np.zeros((K, K), dtype=np.float32)
    sub = LOOP_ROWS if block_size > LOOP_ROWS else block_size
    S = super_rows(block_size, g)
    for s0 in range(0, K, S):
        for i1 in range(s0, min(s0 + S, K), sub):
            i2 = min(i1 + sub, s0 + S, K)
            u[i1:i2, i1:i2] = np.triu(r.standard_normal((i2 - i1, i2 - i1)) * 0.05, 1)
    u[np.arange(K), np.arange(K)] = r.uniform(0.3, 1.5, size=K)
    lo, hi = O.min_max(w.T, "channel")
    s, z = O.qparams(lo, hi, "uint8", False, False)
    return w, u, s.reshape(-1).astype(np.float32), z.reshape(-1).astype(np.int32)


FP32_SHAPES = [(128, 64, 0, 128), (200, 52, 16, 64), (384, 68, 128, 128)]       # K, N, g, block_size


def contraction_case(K=128, N=20, seed=0):
    """One launch in which a fused multiply-add in the row update changes integers.  Scale 1; source row i < K / 2 holds
    t in [1/4, 0.35] with d = 1/4, so its level is the zero point and e = 4 t exactly; its one coefficient c in [1, 1.05] sits on a
    target row j >= K / 2 (a bijection, so the pairs cover slab distances 1 .. 7), and w_j = fl(c e) + 1/2, exact in fp32.  With the
    product rounded first (gptq.py:198-200: a matmul, then a subtraction) the target is exactly 1/2 and rounds to the even level;
    t is drawn so that fl(c e) - c e > 2^-25, and a fused c e leaves 1/2 + 2^-24, which rounds up.
    -> (w, u, init_scale, init_zp, targets [K] bool), uint8."""
    r = np.random.default_rng([K, N, seed, 11])
    half = K // 2
    target_of = half + (np.arange(half) * 5 + 3) % (K - half)
    assert len(set(target_of.tolist())) == half
    w = np.zeros((K, N), dtype=np.float32)
    u = np.zeros((K, K), dtype=np.float32)
    u[np.arange(K), np.arange(K)] = 1.0
    targets = np.zeros(K, dtype=bool)
    for i in range(half):
        j = int(target_of[i])
        c = np.float32(r.uniform(1.0, 1.05))
        t = (r.integers(int(0.25 * 2 ** 18), int(0.35 * 2 ** 18), size=(N, 64)) / 2.0 ** 18)           # candidates per column
        p = np.float64(c) * (4.0 * t)                                                              # exact: 24 x 20 bits
        ok = (p.astype(np.float32).astype(np.float64) - p) > 2.0 ** -25
        assert ok.any(axis=1).all()
        pick = t[np.arange(N), ok.argmax(axis=1)]
        w[i] = pick
        w[j] = ((np.float64(c) * (4.0 * pick)).astype(np.float32).astype(np.float64) + 0.5)
        assert np.array_equal(w[j].astype(np.float64), (np.float64(c) * (4.0 * pick)).astype(np.float32).astype(np.float64) + 0.5)
        u[i, i], u[i, j] = 0.25, c
        targets[j] = True
    return w, u, np.ones(N, dtype=np.float32), (100 + np.arange(N) % 3).astype(np.int32), targets


# ------------------------------------------------------------------------------------ where a wrong output sits
def locate(wrong, K, N, g, block_size, mode="corrected"):
    """wrong [K, N] bool -> list of dict(ord, kernel, i1, slab, r16, c4, count) per (launch, slab, r16, c4) hit, and per column the
    first wrong row with what it follows."""
    rt = routes(K, N, g, block_size, mode)
    rows, cols = np.nonzero(np.asarray(wrong, dtype=bool))
    starts = np.array([la["i1"] for la in rt["launches"]])
    which = np.searchsorted(starts, rows, side="right") - 1
    hits = collections.Counter()
    for rr, cc, l in zip(rows, cols, which):
        la = rt["launches"][l]
        hits[(la["ord"], la["kernel"], la["i1"], int(rr - la["i1"]) // 16, int(rr - la["i1"]) % 16, int(cc) % 4)] += 1
    first = {}
    for rr, cc in zip(rows, cols):
        first.setdefault(int(cc), int(rr))
    follows = collections.Counter()
    for cc, rr in first.items():
        la = rt["launches"][int(np.searchsorted(starts, rr, side="right") - 1)]
        at = "a super-block boundary" if rr == la["i1"] and la["super_start"] else "a block boundary" if rr == la["i1"] and la["block_start"] \
            else "a launch boundary" if rr == la["i1"] else "a slab start" if (rr - la["i1"]) % 16 == 0 else "inside a slab"
        follows[at] += 1
    return [dict(ord=k[0], kernel=k[1], i1=k[2], slab=k[3], r16=k[4], c4=k[5], count=v) for k, v in sorted(hits.items())], dict(follows)


def describe(wrong, K, N, g, block_size, mode="corrected", most=6):
    hits, follows = locate(wrong, K, N, g, block_size, mode)
    if not hits:
        return "no mismatch"
    total = sum(h["count"] for h in hits)
    fields = {k: P.compact(sorted({h[k] for h in hits})) for k in ("ord", "slab", "r16", "c4")}
    kernels = sorted({h["kernel"] for h in hits})
    worst = sorted(hits, key=lambda h: -h["count"])[:most]
    text = "; ".join(f"launch {h['ord']} ({h['kernel']}, rows from {h['i1']}), slab {h['slab']}, r16 {h['r16']}, c4 {h['c4']}: {h['count']}" for h in worst)
    return (f"{total} wrong, kernels {kernels}, launch {fields['ord']}, slab {fields['slab']}, r16 {fields['r16']}, c4 {fields['c4']}; "
            f"a column's first wrong row is at {follows} -- {text}")
