"""What the exact HQQ tests share (test_hqq_cases.py on the CPU, test_hqq_exact_gpu.py on the GPU; test_hqq.py and
test_hqq_half_gpu.py take `integers_given`).

At lp_norm = 1 the exponent of the shrink's power is 0 and the factor exactly 1 on both sides (np.power(x, 0) == 1,
exp2(+-0) == 1); every other step of a round is one correctly rounded fp32 operation, so the kernels owe the oracle's BITS.

`kernel_order_reference`  NumPy restatement of what csrc/hqq.hip documents, written from the kernel's comments and not from the
                          oracle: the row mean by the explicit pairwise tree, the error as a float64 sum / count rounded to fp32,
                          inv_beta = float32(1 / beta) with beta *= kappa in float64.  A second, independent reference:
                          GPU != both -> the kernel is wrong; the two references differ -> the test is wrong.
`decisions_are_robust`    the condition on the INPUTS under which the one thing the two sides do differently -- the sum behind
                          `err < best_err`: float64 in the kernel, fp32 pairwise in NumPy -- cannot change a decision.
`Case` / `AbiCase`        one weight with the oracle's (q, s, z, trace), and `run(ops, **kwargs)`.
"""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

import oq_oracle as O
from conftest import synth_weight

LP_EXACT = 1.0
ROBUST = 1e-5      # about 5 x the worst-case relative error of an fp32 pairwise mean over 2^20 elements, (log2 n + 8) 2^-24


# ------------------------------------------------------------------------------------ the kernel's order, restated
def _leaf(v):
    """pairwise_leaf: v [R, n], n <= 128, all rows at once."""
    n = v.shape[1]
    if n < 8:
        res = np.zeros(v.shape[0], np.float32)
        for i in range(n):
            res = res + v[:, i]
        return res
    r = [v[:, j].copy() for j in range(8)]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] = r[j] + v[:, i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for t in range(i, n):
        res = res + v[:, t]
    return res


def tree_sum(v):
    """pairwise_row: halves above 128 elements, the left one a multiple of 8."""
    n = v.shape[1]
    if n <= 128:
        return _leaf(v)
    n2 = n // 2
    n2 -= n2 % 8
    return tree_sum(v[:, :n2]) + tree_sum(v[:, n2:])


def kernel_order_reference(rows, scale, z0, reduce_range=False, lp_norm=LP_EXACT, beta=1e1, kappa=1.01, iters=20, early_stop=True):
    """(best zero points [R, 1], trace [(err, zero points evaluated)]) in the kernel's operation order."""
    rows = np.ascontiguousarray(rows, np.float32)
    qmin, qmax = (np.float32(v) for v in O.qrange("uint4", False, reduce_range))
    g = rows.shape[1]
    inv = (np.float32(1.0) / scale.astype(np.float32)).reshape(-1, 1)
    expo = np.float32(lp_norm - 1.0)
    z = z0.astype(np.float32).reshape(-1, 1).copy()
    best, best_err, trace = z.copy(), np.inf, []
    b = float(beta)
    for _ in range(iters):
        inv_beta = np.float32(1.0 / b)
        b *= kappa
        wq = np.minimum(np.maximum(np.rint(rows * inv + z), qmin), qmax)
        wr = (wq - z) / inv                                  # div_refined's claim: the correctly rounded quotient
        d = rows - wr
        a = np.abs(d)
        err = float(np.float32(np.sum(a, dtype=np.float64) / float(rows.size)))
        factor = np.exp2(expo * np.log2(a + np.float32(1e-8)))
        we = np.copysign(np.maximum(np.float32(0), a - inv_beta * factor), d)
        v = wq - (rows - we) * inv
        assert v.dtype == np.float32 and factor.dtype == np.float32
        trace.append((err, z.copy()))
        if err < best_err:
            best_err, best = err, z.copy()
        elif early_stop:
            break
        z = (tree_sum(v) / np.float32(g)).reshape(-1, 1)
    return best, trace


def decisions_are_robust(trace):
    """For every round k >= 1: its error is at least ROBUST (relative) away from the best so far, or its zero points are the
    bits of the round that holds `best` (a fixed point: equal inputs give equal errors on both sides)."""
    best_err, best_z = trace[0][0], trace[0][1]
    for err, z in trace[1:]:
        if not (abs(err - best_err) >= ROBUST * err or z.tobytes() == best_z.tobytes()):
            return False
        if err < best_err:
            best_err, best_z = err, z
    return True


def best_round(trace):
    errs = [e for e, _ in trace]
    k, best = 0, np.inf
    for i, e in enumerate(errs):
        if e < best:
            k, best = i, e
    return k


def integers_given(w, scale, z, group_size, reduce_range=False):
    """The finish kernel's contract at ANY lp_norm: q [K, N] = clip(round(rows / s + z)) for the zero points the kernel returned."""
    rows = O.to_rows(np.asarray(w, np.float32), "group", group_size)
    qmin, qmax = O.qrange("uint4", False, reduce_range)
    q = np.clip(np.round(rows / scale.reshape(-1, 1) + z.reshape(-1, 1)), qmin, qmax).astype(np.uint8)
    return O.from_rows(q, w, "group")


def describe_rows(got, want, kgroups):
    """The (column, k-group) rows of two [rows, 1] arrays that differ in bits, with block (col // 256) and lane (col % 64)."""
    bad = np.flatnonzero(got.reshape(-1).view(np.uint32) != want.reshape(-1).view(np.uint32))
    lines = [f"{bad.size} of {got.size} rows differ"]
    for r in bad[:12]:
        col, kg = divmod(int(r), kgroups)
        lines.append(f"  col {col} k-group {kg} block {col // 256} lane {col % 64}: got {got.reshape(-1)[r]!r} want {want.reshape(-1)[r]!r}")
    return "\n".join(lines)


# ------------------------------------------------------------------------------------ weights
def _to_type(w, dtype):
    """fp32 values of `w` rounded to `dtype` (exactly what the device tensor will hold)."""
    if dtype == "float32":
        return w
    import torch
    return torch.from_numpy(w).to(getattr(torch, dtype)).float().numpy()


def make_weight(kind, seed, k, n, g):
    if kind in ("normal", "heavy", "zero_groups"):
        return synth_weight(kind, seed, k, n)
    if kind == "big":
        return synth_weight("normal", seed, k, n) * np.float32(2.0 ** 60)
    if kind == "small":
        return synth_weight("normal", seed, k, n) * np.float32(2.0 ** -60)
    r = np.random.default_rng(seed)
    rows_n = k * n // g
    if kind == "constant":                                  # groups of one repeated value: negative, zero and positive ones
        v = r.standard_normal((rows_n, 1), dtype=np.float32)
        v[::5] = 0.0
        rows = np.repeat(v, g, axis=1)
    elif kind == "ties":
        # range [-8 s, 7 s], s a power of two: scale = s and z0 = 8 exactly, and (m + 0.5) s lands on m + 8.5
        s = np.exp2(r.integers(-6, 3, (rows_n, 1))).astype(np.float32)
        m = r.integers(-8, 7, (rows_n, g)).astype(np.float32)
        half = r.random((rows_n, g)) < 0.7
        rows = (m + np.where(half, np.float32(0.5), r.random((rows_n, g), dtype=np.float32))) * s
        rows[:, 0], rows[:, 1] = -8 * s[:, 0], 7 * s[:, 0]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(rows.astype(np.float32).reshape(n, k).T)


# ------------------------------------------------------------------------------------ cases
PARAMS = {
    "default": dict(),
    "nostop9": dict(early_stop=False, iters=9),
    "one": dict(iters=1),
    "i32": dict(iters=32, early_stop=False),              # the last round count the one-pass route holds
    "i33": dict(iters=33, early_stop=False),              # ... and the first that switches routes
    "rr": dict(reduce_range=True),
    "mse": dict(mse=True),
    "clip": dict(clip_ratio=0.9),
    "fixed": dict(beta=1.0),                              # the oracle stops early on a fixed point: 1 < rounds < iters
    # `best` is neither the first nor the last round evaluated: on the `heavy` matrix with half its range clipped the error falls
    # for five or six rounds and rises again (at lp_norm = 1 it falls monotonically on every unclipped matrix tried)
    "mid": dict(early_stop=False, iters=12, beta=10.0, kappa=0.5, clip_ratio=0.5),
}

Spec = namedtuple("Spec", "kind seed k n group dtype params view")


def spec(g, n, k=None, *, kind="normal", seed=7, dtype="float32", params="default", view="plain", group=None):
    """`g` the rows per group; `group` the group_size ARGUMENT where it is not g (-1, or above K)."""
    return Spec(kind, seed, 3 * g if k is None else k, n, g if group is None else group, dtype, params, view)


def spec_id(s):
    return f"{s.kind}{s.seed}-{s.k}x{s.n}-g{s.group}-{s.dtype}-{s.params}-{s.view}"


class Case:
    """One weight [K, N] (fp32 values, already rounded to the element type) with the oracle's (q, s, z, trace) at lp_norm = 1."""

    lp_norm = LP_EXACT

    def __init__(self, s: Spec, lp_norm=LP_EXACT):
        self.spec, self.lp_norm = s, lp_norm
        self.k, self.n = s.k, s.n
        self.g = s.k if s.group == -1 or s.group > s.k else s.group
        self.kgroups = s.k // self.g
        self.kwargs = dict(PARAMS[s.params])
        self.w = _to_type(make_weight(s.kind, s.seed, s.k, s.n, self.g), s.dtype)
        p = dict(reduce_range=False, clip_ratio=1.0, mse=False, beta=1e1, kappa=1.01, iters=20, early_stop=True)
        p.update(self.kwargs)
        self.p = p
        self.rows = np.ascontiguousarray(O.to_rows(self.w, "group", s.group))
        self.s, self.z0 = O.qparams_from_rows(self.rows, "uint4", "group", False, p["reduce_range"], p["clip_ratio"], p["mse"],
                                              np.float32, np.float32)
        self._optimize()

    def _optimize(self):
        p = self.p
        self.trace = []
        self.z = O.hqq_optimize_zero_point(self.rows, self.s, self.z0, p["reduce_range"], self.lp_norm, p["beta"], p["kappa"], p["iters"],
                                           p["early_stop"], trace=self.trace)
        self.rounds = len(self.trace)
        qmin, qmax = O.qrange("uint4", False, p["reduce_range"])
        q = np.clip(np.round(self.rows / self.s + self.z), qmin, qmax).astype(np.uint8)
        self.q = O.from_rows(q, self.w, "group")

    def kernel_order(self):
        p = self.p
        return kernel_order_reference(self.rows, self.s, self.z0, p["reduce_range"], self.lp_norm, p["beta"], p["kappa"], p["iters"],
                                      p["early_stop"])

    def blob(self):
        return O.matmul_nbits_layout(self.q, self.s, self.z, self.g, 4, zp_is_float=True)[0]

    def device_weight(self):
        """The weight on the device in the case's element type, as the view the case names."""
        import torch
        s = self.spec
        dt = getattr(torch, s.dtype)
        w = torch.from_numpy(self.w).to(dt)
        if s.view == "plain":
            out = w.cuda()
        elif s.view == "ldw":                                # a leading dimension: columns 3 .. 3 + N of a wider matrix
            big = torch.full((s.k, s.n + 7), 777.0, dtype=dt, device="cuda")
            big[:, 3:3 + s.n] = w.cuda()
            out = big[:, 3:3 + s.n]
            assert out.stride(0) == s.n + 7
        else:                                                # "odd": rows that are only 2-byte aligned, an odd leading dimension
            assert s.view == "odd" and dt != torch.float32
            ld = s.n + 5 + (s.n % 2)
            big = torch.full((s.k + 2, ld), 777.0, dtype=dt, device="cuda")
            big[2:, 3:3 + s.n] = w.cuda()
            out = big[2:, 3:3 + s.n]
            assert out.data_ptr() % 4 == 2 and out.stride(0) % 2 == 1
        assert torch.equal(out.float().cpu(), torch.from_numpy(self.w))
        return out

    def run(self, ops, **kwargs):
        """(q or blob, s, z as NumPy arrays, rounds as an int) of `ops.hqq_quantize` on this case."""
        q, s, z, rounds = ops.hqq_quantize(self.device_weight(), self.spec.group, lp_norm=self.lp_norm, **self.kwargs, **kwargs)
        return q.cpu().numpy(), s.cpu().numpy(), z.cpu().numpy(), int(rounds.item())


class AbiCase(Case):
    """Parameters that did not come from RTN, through oq_hqq_optimize_f32 / _h16 themselves: scales log-uniform in
    [2^-20, 2^10] with exact powers of two among them, zero points fractional, negative and above 15; the weight is drawn so that
    w / s + z spans [-1.5, 16.5] (both clamps work)."""

    def __init__(self, s: Spec):
        self.spec, self.lp_norm = s, LP_EXACT
        self.k, self.n, self.g = s.k, s.n, s.group
        self.kgroups = s.k // self.g
        self.kwargs = dict(PARAMS[s.params])
        p = dict(reduce_range=False, beta=1e1, kappa=1.01, iters=20, early_stop=True)
        p.update(self.kwargs)
        self.p = p
        r = np.random.default_rng(s.seed)
        rows_n = s.k * s.n // self.g
        e = r.uniform(-20.0, 10.0, (rows_n, 1))
        e[::3] = np.round(e[::3])
        self.s = np.exp2(e).astype(np.float32)
        if s.kind == "abi":
            self.z0 = r.uniform(-3.0, 19.0, (rows_n, 1)).astype(np.float32)
            assert (self.z0 < 0).any() and (self.z0 > 15).any() and (np.log2(self.s[::3]) % 1 == 0).all()
            level = r.uniform(-1.5, 16.5, (rows_n, self.g)).astype(np.float32)
            rows = ((level - self.z0) * self.s).astype(np.float32)
        else:
            # "abi_div", one round (the given zero points ARE the result): x = m s with x / s == m exactly and z = j + 0.5, so
            # x / s + z is an exact tie -- and x * (1 / s) is one ulp off m in many elements, on either side of it
            assert s.kind == "abi_div" and self.p["iters"] == 1
            self.z0 = (r.integers(-2, 3, (rows_n, 1)) + 0.5).astype(np.float32)
            m = r.integers(0, 16, (rows_n, self.g)).astype(np.float32) - np.floor(self.z0)
            rows = m * self.s
            rows = np.where(rows / self.s == m, rows, np.float32(0))
        self.w = _to_type(np.ascontiguousarray(rows.reshape(s.n, s.k).T), s.dtype)
        self.rows = np.ascontiguousarray(O.to_rows(self.w, "group", self.g))
        self._optimize()

    def workspace_bytes(self):
        from onnx_quantize_amd.hip import _lib as L
        return max(L.load().oq_hqq_workspace_bytes(self.k, self.n, self.g), 256)

    def run(self, ops, **kwargs):
        """As `Case.run`; ``workspace`` (a uint8 device tensor of `workspace_bytes()`) is used where given."""
        import torch
        from onnx_quantize_amd.hip import _lib as L
        lib = L.load()
        w = self.device_weight()
        rows = self.s.size
        scale, zp_in = torch.from_numpy(self.s.reshape(-1)).cuda(), torch.from_numpy(self.z0.reshape(-1)).cuda()
        nbits = kwargs.get("layout", "kn") == "nbits"
        q = torch.zeros((self.n, self.kgroups, self.g // 2) if nbits else (self.k, self.n), dtype=torch.uint8, device="cuda")
        zp = torch.zeros(rows, dtype=torch.float32, device="cuda")
        rounds = torch.zeros(1, dtype=torch.int32, device="cuda")
        ws = kwargs.get("workspace")
        if ws is None:
            ws = torch.zeros(self.workspace_bytes(), dtype=torch.uint8, device="cuda")
        ptr = lambda t: C.c_void_p(t.data_ptr())     # noqa: E731
        p = self.p
        tail = (self.k, self.n, w.stride(0), self.g, int(p["reduce_range"]), ptr(scale), ptr(zp_in), float(self.lp_norm), float(p["beta"]),
                float(p["kappa"]), int(p["iters"]), int(p["early_stop"]), int(bool(kwargs.get("per_round_launches", False))), ptr(q),
                L.OQ_LAYOUT_NBITS if nbits else L.OQ_LAYOUT_KN, ptr(zp), ptr(rounds), ptr(ws), ws.numel(),
                C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if self.spec.dtype == "float32":
            L.check(lib.oq_hqq_optimize_f32(ptr(w), *tail))
        else:
            L.check(lib.oq_hqq_optimize_h16(ptr(w), L.WTYPE_CODE[self.spec.dtype], *tail))
        return q.cpu().numpy(), scale.cpu().numpy().reshape(-1, 1), zp.cpu().numpy().reshape(-1, 1), int(rounds.item())


@functools.lru_cache(maxsize=None)
def case(s: Spec):
    """The case of a spec, made once per process: the oracle's result is shared by every test and route that names the spec."""
    return AbiCase(s) if s.kind.startswith("abi") else Case(s)


# --- the exact tier -------------------------------------------------------------------------------------------------
TILE_GROUPS = (16, 32, 64, 128)
EDGE_N = (1, 37, 255, 256, 257, 520)                      # the edges of the 256-column block and of the `live` clamp
GENERAL_GROUPS = (4, 12, 20, 24, 40, 136, 264, 300, 520)  # plain loop, tail loop, one halving, two (300 -> 144 + 156 -> 72 + 84), ...
PARAM_SETS = tuple(PARAMS)
KINDS = ("heavy", "zero_groups", "constant", "ties", "big", "small")
HALF = ("float16", "bfloat16")

# register-tile groups, both routes: every block edge, one k-group and three
# (seeds other than 7 below: the first seed whose oracle trace meets `decisions_are_robust`)
TILE = [spec(g, n, k, seed=8 if (n, k) == (1, g) and g < 128 else 7) for g in TILE_GROUPS for n in EDGE_N for k in (g, 3 * g)]
# g = 256: fp32 runs pairwise_row on the per-round route; the 2-byte types the packed one-pass tile and the per-round route
G256 = [spec(256, n, k, dtype=dt) for dt in ("float32",) + HALF for n, k in ((37, 256), (257, 768))]
# general groups, per-round route by themselves; a leaf of exactly 128 is 264 -> 128 + 136 and 520 -> 256 + 264 -> (128 + 128) + ...
GENERAL = [spec(g, n, seed=8 if (g, n) == (24, 37) else 7) for g in GENERAL_GROUPS for n in (37, 257)]
GENERAL += [spec(96, 37, 96, group=-1), spec(96, 37, 96, group=200)]
# every parameter set on a register-tile group and on a general one
PARAMETERS = [spec(g, 257, params=p) for g in (64, 24) for p in PARAM_SETS if p not in ("default", "fixed", "mid")]
PARAMETERS += [spec(16, 257, params="fixed", seed=9), spec(24, 257, params="fixed")]
PARAMETERS += [spec(g, 257, params="mid", kind="heavy") for g in (64, 24)]
DATA = [spec(g, 257, kind=kind, seed={("small", 32): 8, ("small", 40): 9}.get((kind, g), 7)) for g in (32, 40) for kind in KINDS]
TYPES = [spec(g, 257, dtype=dt) for dt in HALF for g in (16, 128, 40)]
VIEWS = [spec(g, 257, view="ldw") for g in (64, 24)] + [spec(g, 37, dtype=dt, view="odd") for dt in HALF for g in (32, 256, 24)]
ABI = [spec(g, 257, kind="abi", dtype=dt) for g in (64, 24) for dt in ("float32", "bfloat16")] + [spec(256, 37, kind="abi", dtype="float16", seed=24)]
ABI += [spec(g, 257, kind="abi_div", params="one") for g in (64, 24)]      # the finish kernel's division on exact ties
ABI += [spec(64, 257, kind="abi", params=p) for p in ("i32", "i33")]       # test_32_rounds_are_the_last_the_one_pass_route_holds

EXACT = TILE + G256 + GENERAL + PARAMETERS + DATA + TYPES + VIEWS + ABI
assert len(set(EXACT)) == len(EXACT)


def routes(s: Spec):
    """The routes a spec is run on: the default one, and the forced per-round route where the default is the one-pass kernel."""
    g = s.k if s.group == -1 or s.group > s.k else s.group
    tile = g in TILE_GROUPS or (g == 256 and s.dtype != "float32")
    return (False, True) if tile and PARAMS[s.params].get("iters", 20) <= 32 else (False,)


# exact integers at every lp_norm: a ragged N, a g = 256 half and a general g, at the norms whose power is not reproducible
ANY_NORM = [(s, lp) for s in (spec(64, 257), spec(256, 37, 256, dtype="bfloat16"), spec(40, 257)) for lp in (0.5, 0.7)]


@functools.lru_cache(maxsize=None)
def case_at(s: Spec, lp_norm: float):
    return Case(s, lp_norm)
