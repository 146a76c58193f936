"""What the exact tests of the GPTQ factor share (test_gptq_factor_cases.py, test_gptq_factor_exact_gpu.py): plain numpy, no library
call.

`exact_case`   a seeded Hessian whose inverse factor U is owed bit for bit, with its closed form;
`exact_ok`     the chain of csrc/factor.hip restated product by product on the host: the largest sum |a| |b| of any product, in units
               of that product's dyadic grid, and the widest operand of any fp16-piece leg in significant bits;
`pivot_case`   the same Hessian with one pivot of the reversed space spoiled (zero, negative, NaN);
`legs`         the host dispatch of `factor_batched` restated as the list of its launches;
`locate`       wrong elements of U -> the launch that wrote them; `describe` as text.

Why the factor can be exact.  The kernel factors P = J (H + d I) J = L' L'^T and returns U = J L'^-1 J.  Give every index a class
c(i) in {0, 1, 2}; E is strictly lower triangular with small integers only where c(i) > c(j), so E^3 = 0; D = diag(2^e), e in
{0, 1, 2}; L' = (I + E) D.  Then L'^-1 = D^-1 (I - E + E^2) has multiples of 1/4, P is an integer matrix, and every diagonal block
of L' has the same structure, so each 32-row and 128-row factor and inverse, each panel, each trailing block and each level of the
recursive doubling is a matrix of dyadic rationals on a known grid: 1 for L' and the trailing blocks of P, 1/4 for the inverses and
for L21 X11, 1/16 for the products of two of those.  A sum of multiples of g whose absolute terms add up to less than 2^24 g is an
fp32 number at every partial sum, in whatever order a register loop, an LDS product, the fp32 MFMA GEMM or the fp16-piece GEMM adds:
nothing is ever rounded.  The pivots are 4^e, their roots 2^e, the divisions by them exact.  On the fp16-piece legs an operand
element with at most 11 significant bits is its own first piece, the second piece is zero, and the term the kernels drop (lo lo)
vanishes with it.  `exact_ok` computes both figures for a case; nothing here assumes them."""
import collections
import functools

import numpy as np

NB = 128                        # kNB: block size of the factorisation
SB = 32                         # kSB: register sub-block of the diagonal kernel
OUTER = 4 * NB                  # kOuter: rows of an outer panel
PIECE_UPDATE_MIN = 1024         # kPieceUpdateMin: narrower deferred squares stay on the fp32 GEMM
PIECE_INVERSE_MIN = 2048        # kPieceInverseMin: inverse levels from this block size on run on fp16 pieces
GEMM_TILE = 128                 # kBM = kBN of gemm_tn.hip
PIECE_TILE = 256                # kST of syrk_bf16x3.hip
PIECE_ROWS = 32                 # F16Stage::ROWS
LIMIT = float(1 << 24)


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------ the recipe
class Case:
    """K, h [K, K] fp32 (what the kernel is given), percdamp (fp32 value as a Python float), damp (the dyadic d it yields), u [K, K]
    fp32 (owed), l / linv [K, K] float64 (L' and L'^-1, reversed index space), dead (indices of H), info (owed), name."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _matmul_exact(a, b):
    """a @ b for integer-valued matrices in float32 BLAS, with the condition under which that is exact asserted"""
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    assert float((np.abs(a32) @ np.abs(b32)).max(initial=0.0)) < LIMIT
    return (a32 @ b32).astype(np.float64)


def damp_for(h, d):
    """-> the fp32 percdamp with fl32(percdamp * fl32(t / K)) == d, t = sum of diag(h) (damp_kernel); None if no neighbour has it"""
    K = h.shape[0]
    t = np.float32(np.diagonal(h).astype(np.float64).sum())
    mean = np.float32(t / np.float32(K))
    p = np.float32(np.float64(d) / np.float64(mean))
    cands = [p]
    up = dn = p
    for _ in range(8):
        up, dn = np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf))
        cands += [up, dn]
    for q in cands:
        if np.float32(q * mean) == np.float32(d):
            return float(q)
    return None


@functools.lru_cache(maxsize=None)
def exact_case(K, seed, damp=None, dead=(), density=0.25, amp=1):
    rng = np.random.default_rng([seed, K])
    cls = rng.integers(0, 3, size=K)
    e = rng.integers(0, 3, size=K)
    mag = rng.integers(1, amp + 1, size=(K, K)) * rng.choice([-1, 1], size=(K, K))
    E = np.where((rng.random((K, K)) < density) & (cls[:, None] > cls[None, :]), mag, 0).astype(np.float64)
    E = np.tril(E, -1)
    for i in dead:                      # row and column e_i: index K - 1 - i of the reversed space
        j = K - 1 - i
        E[j, :] = 0.0
        E[:, j] = 0.0
        e[j] = 0
    d = np.exp2(e.astype(np.float64))
    eye = np.eye(K)
    l = (eye + E) * d[None, :]
    linv = (eye - E + _matmul_exact(E, E)) / d[:, None]
    p = _matmul_exact(l, l.T)
    h = np.ascontiguousarray(p[::-1, ::-1])
    percdamp = 0.0
    if damp is not None:                # a dyadic d, or candidates of which the first with an fp32 percdamp is taken
        assert not dead
        found = [(dd, damp_for(h - dd * eye, dd)) for dd in (damp if isinstance(damp, tuple) else (damp,))]
        found = [(dd, pp) for dd, pp in found if pp is not None]
        assert found, "no fp32 percdamp yields any of these damps"
        damp, percdamp = found[0]
        h = h - damp * eye
    for i in dead:
        assert h[i, i] == 1.0
        h[i, i] = 0.0
    u = np.ascontiguousarray(linv[::-1, ::-1])
    h32, u32 = h.astype(np.float32), u.astype(np.float32)
    name = f"K{K}-s{seed}" + (f"-d{damp}" if damp is not None else "") + (f"-dead{len(dead)}" if dead else "")
    return Case(K=K, h=h32, percdamp=percdamp, damp=0.0 if damp is None else float(damp), u=u32, l=l, linv=linv, dead=tuple(dead), info=0,
                name=name, density=density, amp=amp)


def reversed_p(case):
    """P = J (H + d I) J with the dead fix, in float64: what the Cholesky loop starts from"""
    h = case.h.astype(np.float64)
    for i in case.dead:
        h[i, i] = 1.0
    return np.ascontiguousarray(h[::-1, ::-1]) + case.damp * np.eye(case.K)


def pivot_case(case, pivots, kind="zero"):
    """`case` with pivot j of the reversed space (0-based) spoiled; `pivots` is j or a list of (j, kind), the first of which is owed:
    info = j + 1, U = I.  zero: P[j][j] is lowered by exactly L'[j][j]^2; negative: by twice that; nan: P[j][j-1] and its mirror are
    NaN, which leaves the diagonal (and the damp sum) finite -- at j = 0 there is no such entry and P[0][0] itself is NaN.  Leading
    minors in front of j are unchanged."""
    K = case.K
    items = [(pivots, kind)] if np.isscalar(pivots) else list(pivots)
    h = case.h.copy()
    for j, kd in items:
        i = K - 1 - j
        ljj2 = np.float32(case.l[j, j] ** 2)
        if kd == "zero":
            h[i, i] -= ljj2
        elif kd == "negative":
            h[i, i] -= np.float32(2) * ljj2
        elif kd == "nan":
            if j == 0:
                h[i, i] = np.nan
            else:
                h[i, i + 1] = np.nan
                h[i + 1, i] = np.nan
        else:
            raise ValueError(kd)
    first = min(j for j, _ in items)
    return Case(K=K, h=h, percdamp=case.percdamp, damp=case.damp, u=np.eye(K, dtype=np.float32), l=case.l, linv=case.linv, dead=case.dead,
                info=first + 1, name=case.name + "-" + "+".join(f"{kd}{j}" for j, kd in items), density=case.density, amp=case.amp)


# ------------------------------------------------------------------------------------ the host dispatch
def _vec(ld, cols, base, batch_strides):
    """launch_gemm_tn's test for the 16-byte loads of one operand (the workspace is 256-byte aligned)"""
    return ld % 4 == 0 and cols % 4 == 0 and base % 4 == 0 and all(s % 4 == 0 for s in batch_strides)


def _padded(nbytes, align=256):
    return ceil_div(nbytes, align) * align


def _piece_item_bytes(T, cols):
    return 16384 + ceil_div(T, PIECE_ROWS) * 4 * 2 * ceil_div(cols, PIECE_TILE) * PIECE_TILE * 16


def pieces_ok(K, count, method):
    """factor_batched: the X region must hold the deferred update's table (128 bytes per matrix) and pieces"""
    need = _padded(count * 128) + _padded(count * _piece_item_bytes(OUTER, K)) + 256
    return method != "f32" and need <= count * _padded(K * K * 4)


def legs(K, count=1, method="auto"):
    """-> list of dicts, one per launch (group) of `factor_batched`, in order.  kind: diag | panel | strip | deferred | level."""
    out = []
    ms, ds = _padded(K * K * 4) // 4, _padded(ceil_div(K, NB) * NB * NB * 4) // 4
    outer = (lambda *s: s) if count > 1 else (lambda *s: ())
    pok = pieces_ok(K, count, method)
    for O in range(0, K, OUTER):
        pend = min(O + OUTER, K)
        for o in range(O, pend, NB):
            kb, n = o // NB, min(K - o, NB)
            rest = K - o - n
            out.append(dict(kind="diag", kb=kb, n=n))
            if rest <= 0:
                break
            out.append(dict(kind="panel", kb=kb, M=n, N=rest, Kd=n,
                            arm_a="vector" if _vec(NB, n, kb * NB * NB, outer(ds)) else "scalar",
                            arm_b="vector" if _vec(K, rest, o * K + o + n, outer(ms)) else "scalar"))
            strip = pend - (o + n)
            if strip > 0:
                base = o * K + o + n
                out.append(dict(kind="strip", kb=kb, M=strip, N=rest, Kd=n,
                                arm_a="vector" if _vec(K, strip, base, outer(ms)) else "scalar",
                                arm_b="vector" if _vec(K, rest, base, outer(ms)) else "scalar"))
        rest2 = K - pend
        if rest2 >= PIECE_UPDATE_MIN and pok:
            tn = ceil_div(rest2, PIECE_TILE)
            out.append(dict(kind="deferred", leg="pieces", O=O, pend=pend, n=rest2, Kd=pend - O, tiles=tn, upper_tiles=tn * (tn + 1) // 2,
                            padded=rest2 % PIECE_TILE != 0, super_tiles=1))
        elif rest2 > 0:
            tn = ceil_div(rest2, GEMM_TILE)
            base = O * K + pend
            arm = "vector" if _vec(K, rest2, base, outer(ms)) else "scalar"
            out.append(dict(kind="deferred", leg="gemm_tn", O=O, pend=pend, n=rest2, Kd=pend - O, tiles=tn, upper_tiles=tn * (tn + 1) // 2,
                            padded=rest2 % GEMM_TILE != 0, super_tiles=ceil_div(tn, 8), arm_a=arm, arm_b=arm))
    inv_pieces = any(b >= PIECE_INVERSE_MIN for b in _levels(K))
    for b in _levels(K):
        npairs, full = (K - b + 2 * b - 1) // (2 * b), K // (2 * b)
        for part in range(2):
            first, pairs = (0, full) if part == 0 else (full, npairs - full)
            if pairs <= 0:
                continue
            o1 = first * 2 * b
            o2 = o1 + b
            b2 = b if part == 0 else K - o2
            leg = "pieces" if b >= PIECE_INVERSE_MIN and pok and inv_pieces else "gemm_tn"
            d = dict(kind="level", b=b, shape="full" if part == 0 else "ragged", first=first, pairs=pairs, b2=b2, leg=leg)
            if leg == "gemm_tn":
                st = (2 * b * (K + 1),) if pairs > 1 else ()
                d.update(arm_a1="vector" if _vec(K, b2, o1 * K + o2, st + outer(ms)) else "scalar",
                         arm_b1="vector" if _vec(K, b, o1 * K + o1, st + outer(ms)) else "scalar",
                         arm_a2="vector" if _vec(K, b2, o2 * K + o2, st + outer(ms)) else "scalar",
                         arm_b2="vector" if _vec(b, b, first * b * b, ((b * b,) if pairs > 1 else ()) + outer(ms)) else "scalar")
            out.append(d)
    return out


def _levels(K):
    b = NB
    while b < K:
        yield b
        b *= 2


# ------------------------------------------------------------------------------------ the chain restated
Exactness = collections.namedtuple("Exactness", "units piece_bits worst x")


class _Tally:
    def __init__(self):
        self.units, self.worst, self.bits = 0.0, "", 0

    def product(self, what, a, b, grid, c_in=None):
        """one product sum_k a[i][k] b[k][j] (+ c_in) whose terms are multiples of `grid`"""
        if a.size == 0 or b.size == 0:
            return
        mass = np.abs(a) @ np.abs(b)
        if c_in is not None:
            mass = mass + np.abs(c_in)
        v = float(mass.max()) / grid
        if v > self.units:
            self.units, self.worst = v, what

    def piece_operand(self, x):
        """significant bits of the widest element: all are multiples of 1/16 here"""
        v = np.abs(x * 16.0).astype(np.int64)
        v = v[v != 0]
        if v.size:
            self.bits = max(self.bits, int((v // (v & -v)).max()).bit_length())


def _diag_block(A, n, tally, kb):
    """chol_diag_kernel on the n x n block A (float64), padded with the identity to 128 -> (L [n, n], inv(L) [n, n])"""
    a = np.eye(NB)
    a[:n, :n] = A
    m = np.zeros((NB, NB))
    for so in range(0, NB, SB):
        s_ = slice(so, so + SB)
        sub = a[s_, s_]
        # chol32_regs: left-looking inside the sub-block; the pivots are squares of powers of two
        lsub = np.zeros((SB, SB))
        for j in range(SB):
            sv = sub[:, j] - lsub[:, :j] @ lsub[j, :j]
            piv = sv[j]
            assert piv > 0 and np.exp2(2 * np.round(np.log2(piv) / 2)) == piv, f"block {kb}: pivot {so + j} is not a power of four"
            lsub[j:, j] = sv[j:] / np.sqrt(piv)
        strict = np.tril(lsub, -1)
        tally.product(f"diag {kb} sub-block {so // SB} factor", strict, strict.T, 1.0, np.abs(sub))
        # inv32_regs: forward substitution, column by column over the lanes
        msub = np.zeros((SB, SB))
        for i in range(SB):
            msub[i, :] = ((np.arange(SB) == i) - lsub[i, :i] @ msub[:i, :]) / lsub[i, i]
        tally.product(f"diag {kb} sub-block {so // SB} inverse", strict, msub, 0.25, np.eye(SB))
        a[s_, s_] = np.tril(lsub) + np.triu(sub, 1)
        m[s_, s_] = msub
        ro = so + SB
        if ro < NB:
            a21 = a[ro:, s_]
            tally.product(f"diag {kb} panel under sub-block {so // SB}", a21, msub.T, 0.25)
            l21 = a21 @ msub.T
            a[ro:, s_] = l21
            tally.product(f"diag {kb} trailing behind sub-block {so // SB}", l21, l21.T, 1.0, a[ro:, ro:])
            a[ro:, ro:] -= l21 @ l21.T
    for ro in range(SB, NB, SB):
        r_ = slice(ro, ro + SB)
        x11 = np.tril(m[:ro, :ro])
        tally.product(f"diag {kb} off-diagonal inverse row {ro // SB} (L X)", a[r_, :ro], x11, 0.25)
        s = a[r_, :ro] @ x11
        tally.product(f"diag {kb} off-diagonal inverse row {ro // SB} (X S)", m[r_, r_], s, 1.0 / 16)
        m[r_, :ro] = -(m[r_, r_] @ s)
    return np.tril(a)[:n, :n], np.tril(m)[:n, :n]


def exact_ok(case, method="auto", count=1):
    """The chain of `factor_batched` on `case` in float64, launch by launch -> Exactness(units, piece_bits, worst, x): the largest
    sum |a| |b| (+ |c|) of any product in units of its grid with the product that has it, the widest operand element of any
    fp16-piece leg in significant bits (0: no such leg), and the X = L'^-1 the chain arrives at."""
    K = case.K
    t = _Tally()
    P = reversed_p(case)
    Lt = np.zeros((K, K))
    dinv = {}
    if case.percdamp != 0.0:            # damp_kernel adds the diagonal up in fp32: multiples of 1/8 (DAMPS)
        t.product("damp sum", np.abs(np.diagonal(case.h).astype(np.float64))[None, :], np.ones((K, 1)), 0.125)
    for leg in legs(K, count, method):
        kind = leg["kind"]
        if kind == "diag":
            o, n = leg["kb"] * NB, leg["n"]
            l, m = _diag_block(P[o:o + n, o:o + n], n, t, leg["kb"])
            Lt[o:o + n, o:o + n] = l.T
            dinv[leg["kb"]] = m
        elif kind == "panel":
            o, n = leg["kb"] * NB, leg["M"]
            m, b = dinv[leg["kb"]], P[o:o + n, o + n:]
            t.product(f"panel {leg['kb']}", m, b, 0.25)
            Lt[o:o + n, o + n:] = m @ b
        elif kind == "strip":
            o, n = leg["kb"] * NB, leg["Kd"]
            a, b = Lt[o:o + n, o + n:o + n + leg["M"]], Lt[o:o + n, o + n:]
            c = P[o + n:o + n + leg["M"], o + n:]
            t.product(f"strip {leg['kb']}", a.T, b, 1.0, c)
            c -= a.T @ b
        elif kind == "deferred":
            O, pend = leg["O"], leg["pend"]
            a = Lt[O:pend, pend:]
            c = P[pend:, pend:]
            t.product(f"deferred square behind {pend} ({leg['leg']})", a.T, a, 1.0, c)
            if leg["leg"] == "pieces":
                t.piece_operand(a)
            c -= a.T @ a
        else:
            break
    X = np.zeros((K, K))
    for kb, m in dinv.items():
        X[kb * NB:kb * NB + m.shape[0], kb * NB:kb * NB + m.shape[0]] = m
    for leg in legs(K, count, method):
        if leg["kind"] != "level":
            continue
        b, b2 = leg["b"], leg["b2"]
        for p in range(leg["first"], leg["first"] + leg["pairs"]):
            o1 = p * 2 * b
            o2 = o1 + b
            l21 = Lt[o1:o2, o2:o2 + b2].T
            x11, x22 = X[o1:o2, o1:o2], X[o2:o2 + b2, o2:o2 + b2]
            t.product(f"level {b} {leg['shape']} pair {p} (L21 X11, {leg['leg']})", l21, x11, 0.25)
            s = l21 @ x11
            t.product(f"level {b} {leg['shape']} pair {p} (X22 S, {leg['leg']})", x22, s, 1.0 / 16)
            if leg["leg"] == "pieces":
                for op in (l21, x11, x22, s):
                    t.piece_operand(op)
            X[o2:o2 + b2, o1:o2] = -(x22 @ s)
    return Exactness(t.units, t.bits, t.worst, X)


# ------------------------------------------------------------------------------------ wrong elements -> the launch that wrote them
def locate(K, wrong):
    """wrong [K, K] bool over U -> Counter of leg names.  U[a][b] = X[K-1-a][K-1-b]: X is lower triangular, its diagonal 128-blocks
    come from chol_diag_kernel (a 32-sub-block of the register loops or a block row of the off-diagonal phase), block (I, J), I > J,
    from the level b at which I and J first share a pair; everything above the diagonal of X is written as zero by the last kernel."""
    r, c = np.nonzero(np.asarray(wrong)[::-1, ::-1])
    out = collections.Counter()
    if r.size == 0:
        return out
    I, J = r // NB, c // NB
    upper, diag = c > r, (I == J) & (c <= r)
    level = ~upper & ~diag
    keys = np.zeros((r.size, 5), dtype=np.int64)            # (kind, block or level, pair or sub-block row, tile row, tile column)
    keys[upper, 0] = 0
    ri, ci = (r % NB) // SB, (c % NB) // SB
    keys[diag] = np.stack([np.ones(diag.sum(), dtype=np.int64), I[diag], ri[diag], (ri == ci)[diag].astype(np.int64), 0 * I[diag]], axis=1)
    if level.any():
        rl, cl = r[level], c[level]
        b = NB << np.floor(np.log2(I[level] ^ J[level])).astype(np.int64)      # the level at which I and J first share a pair
        pair = rl // (2 * b)
        o1 = pair * 2 * b
        keys[level] = np.stack([2 + 0 * b, b, pair, (rl - o1 - b) // NB, (cl - o1) // NB], axis=1)
    codes = (((keys[:, 0] << 20 | keys[:, 1]) << 12 | keys[:, 2]) << 12 | keys[:, 3]) << 12 | keys[:, 4]       # K < 2^19
    for code, n in zip(*np.unique(codes, return_counts=True)):
        code = int(code)
        kind, x, y, z, w = code >> 56, (code >> 36) & 0xFFFFF, (code >> 24) & 4095, (code >> 12) & 4095, code & 4095
        if kind == 0:
            name = "zero triangle (finish_factor_kernel)"
        elif kind == 1:
            name = f"diag block {x}, " + (f"sub-block {y}" if z else f"off-diagonal phase row {y}")
        else:
            name = f"level {x}, {'full' if y < K // (2 * x) else 'ragged'} pair {y}, tile ({z}, {w})"
        out[name] += int(n)
    return out


def describe(K, wrong, limit=6):
    found = locate(K, wrong)
    parts = [f"{name}: {n} wrong" for name, n in found.most_common(limit)]
    if len(found) > limit:
        parts.append(f"... {len(found) - limit} more regions")
    return "; ".join(parts) if parts else "nothing wrong"


# ------------------------------------------------------------------------------------ the cases of the GPU file
# width -> (density, amp): fewer and smaller entries as the sums get longer
WIDTHS = (1, 33, 96, 128, 129, 256, 388, 515, 640, 1100, 1536, 1664, 2176, 4096)
TWO_METHODS_FROM = 1536
DAMPED = (1, 96, 129, 256, 388, 515, 640, 1100, 1536, 1664, 2176)          # widths that also run with an exact non-zero damp


def recipe(K):
    if K <= 640:
        return dict(density=0.5, amp=2)
    if K <= 1664:
        return dict(density=0.25, amp=1)
    return dict(density=0.125, amp=1)


DAMPS = (0.25, 0.75, 0.375, 0.625, 1.25)            # the product percdamp * mean hits a given d for about two means in three


def width_case(K, damped=False, seed=1, dead=()):
    return exact_case(K, seed, DAMPS if damped else None, tuple(dead), **recipe(K))


def methods_of(K):
    return ("auto", "f32") if K >= TWO_METHODS_FROM else ("auto",)
