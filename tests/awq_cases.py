"""Inputs and CPU-side conditions of the AWQ edge tests, shared by tests/test_awq_cases.py (CPU: the conditions on the oracle alone)
and tests/test_awq_edges_gpu.py (GPU: the searches against the oracle).  An ordinary module, NumPy and the oracle only.

A SPOTLIGHT case puts (nearly) all of the loss ||X D||^2 into a region of D = W - W^ that one kernel route could get wrong while
the whole-matrix loss of an i.i.d. input would hide it:

* column spotlight: `w[:, region] *= 1e3`.  Group and channel maxima are per column, so the weight statistic `ws` (and with it
  every candidate scale) is that of the plain input; the region's columns carry 1e6 times the loss of any other column.
* row spotlight: `x[:, k] = 0` outside the region.  Those channels are dead (mean |x| = 0, the candidate scale clamps at 1e-4) and
  contribute exactly nothing to X D; the loss comes from the region's rows of D alone.

`conditions` states what makes such a case a test, in float64 from the oracle's own D of every candidate of both searches:
the region's share of the loss, and that the oracle's fp32 loss is not dominated by cancellation."""
from collections import namedtuple

import numpy as np

import oq_oracle as O

AMPLIFY = 1e3
SHARE_COLS = 0.999          # least share of the loss inside a column region
CONDITIONING = 2e-4         # oracle fp32 loss vs float64, a tenth of the 2e-3 loss bar

Case = namedtuple("Case", "name kind x w region qtype strategy g sym reduce_range")

# name: (kind, seed, T, K, N, qtype, strategy, g, symmetric, reduce_range, (first, last + 1) of the region)
# The seed is the case's number, except C2: with seed 2 its single column holds 0.99896 of the loss, below SHARE_COLS; 12 (the next
# tried) gives 0.99954.
SPOTLIGHTS = {
    "C1": ("cols", 1, 48, 64, 260, "uint4", "group", 32, False, False, (256, 260)),
    "C2": ("cols", 12, 48, 64, 257, "int8", "channel", -1, True, False, (256, 257)),
    "C3": ("cols", 3, 48, 64, 258, "uint4", "group", 8, False, False, (256, 258)),
    "C4": ("cols", 4, 64, 256, 516, "int4", "group", 128, False, False, (512, 516)),
    "C5": ("cols", 5, 48, 64, 260, "uint4", "group", 32, False, False, (0, 4)),
    "C6": ("cols", 6, 48, 64, 520, "uint4", "group", 16, False, False, (256, 260)),
    "R1": ("rows", 1, 48, 100, 24, "int8", "channel", -1, False, False, (96, 100)),
    "R2": ("rows", 2, 48, 176, 64, "uint4", "group", 16, False, False, (160, 176)),
    "R3": ("rows", 3, 48, 192, 64, "uint4", "group", 16, False, False, (176, 192)),
    "R4": ("rows", 4, 48, 64, 64, "int4", "group", 32, True, False, (0, 32)),
    "R5": ("rows", 5, 48, 68, 36, "uint8", "tensor", -1, False, False, (64, 68)),
    "R6": ("rows", 6, 48, 256, 64, "uint4", "group", 128, False, False, (128, 256)),
    # R2's and R3's shapes and regions on fresh inputs: int8 per channel with the reduced range (array route only)
    "R2r": ("rows", 22, 48, 176, 64, "int8", "channel", -1, False, True, (160, 176)),
    "R3r": ("rows", 23, 48, 192, 64, "int8", "channel", -1, False, True, (176, 192)),
}
ALL_ROUTES = [n for n in SPOTLIGHTS if not n.endswith("r")]


def inputs(seed, t, k, n):
    """tests/test_preprocessing.py::_inputs with the activations as [T, K] (the same stream of random numbers)."""
    r = np.random.default_rng(seed)
    x = r.standard_normal((t, k)).astype(np.float32) * r.uniform(0.1, 4, k).astype(np.float32)
    w = (r.standard_normal((k, n)) * 0.05).astype(np.float32)
    return x, w


_cache = {}


def spotlight(name):
    """The case, made once; its arrays are shared and must stay unchanged."""
    if name not in _cache:
        kind, seed, t, k, n, qtype, strategy, g, sym, rr, (a, b) = SPOTLIGHTS[name]
        x, w = inputs(seed, t, k, n)
        if kind == "cols":
            w[:, a:b] *= np.float32(AMPLIFY)
        else:
            x[:, :a] = 0.0
            x[:, b:] = 0.0
        x.setflags(write=False)
        w.setflags(write=False)
        _cache[name] = Case(name, kind, x, w, (a, b), qtype, strategy, g, sym, rr)
    return _cache[name]


def tiled_for_gram(x, k):
    """`x` repeated along T until T >= 3 K (the searches' Gram route): the loss (a mean over rows) and mean |x| are unchanged."""
    reps = -(-3 * k // x.shape[0])
    out = np.tile(x, (reps, 1))
    assert out.shape[0] >= 3 * k
    return out


def candidate_scales(x, w, strategy, g, n_grid=20):
    """awq.py:143-150 for every grid point, as O.awq_scale_search builds them: [n_grid, K] fp32."""
    act, ws = O.awq_activation_scale(x), O.awq_weight_scale(w, strategy, g)
    rows = []
    for i in range(n_grid):
        ratio = i * 1 / n_grid
        scale = np.clip(np.power(act, ratio) / np.power(ws, (1 - ratio)), 1e-4, None)
        rows.append(scale / np.sqrt(np.max(scale) * np.min(scale)))
    out = np.stack(rows)
    assert out.dtype == np.float32
    return out


def scale_residuals(x, w, qtype, strategy, g, sym=False, reduce_range=False, n_grid=20):
    """D = W - W^ of every candidate of the scale search, by the oracle's own steps (O.awq_scale_search's loop body)."""
    out = []
    for scale in candidate_scales(x, w, strategy, g, n_grid):
        col = scale.reshape(-1, 1)
        q, s, z = O.rtn_quantize(w * col, qtype, strategy, g, sym, reduce_range)
        out.append(w - O.dequantize(q, s, z, rows_of=strategy, group_size=g) / col)
    return out


def clip_residuals(w, qtype, strategy, g, sym=False, reduce_range=False):
    """D = W - W^ of the ten candidates of the clip search (O.awq_clip_search's loop body)."""
    out = []
    for i in range(10):
        q, s, z = O.rtn_quantize(w, qtype, strategy, g, sym, reduce_range, clip_ratio=1 - i / 100)
        out.append(w - O.dequantize(q, s, z, rows_of=strategy, group_size=g))
    return out


_oracle = {}


def oracle(name):
    """(winning scale, scale-search losses, clip ratio, clip-search losses) of the oracle on a spotlight case, computed once."""
    if name not in _oracle:
        c = spotlight(name)
        es, el = O.awq_scale_search(c.x, c.w, c.qtype, c.strategy, c.g, c.sym, c.reduce_range)
        er, ecl = O.awq_clip_search(c.x, c.w, c.qtype, c.strategy, c.g, c.sym, c.reduce_range)
        _oracle[name] = (es, el, er, ecl)
    return _oracle[name]


_conditions = {}


def conditions(name):
    """Computed once per case.  (least region share, largest |fp32 loss / float64 loss - 1|) over the 20 + 10 candidates of both searches.

    The share of a column region is sum_{n in region} ||X d_n||^2 / ||X D||^2; that of a row region is
    1 - ||X[:, outside] D[outside]||^2 / ||X D||^2, which is exactly 1 when every outside channel of X is zero."""
    if name in _conditions:
        return _conditions[name]
    c = spotlight(name)
    a, b = c.region
    _, el, _, ecl = oracle(name)
    x64 = c.x.astype(np.float64)
    ds = scale_residuals(c.x, c.w, c.qtype, c.strategy, c.g, c.sym, c.reduce_range) + clip_residuals(c.w, c.qtype, c.strategy, c.g, c.sym, c.reduce_range)
    share, cond = 1.0, 0.0
    for d, loss32 in zip(ds, list(el) + list(ecl)):
        assert np.isfinite(d).all(), name
        d64 = d.astype(np.float64)
        per_col = ((x64 @ d64) ** 2).sum(0)
        total = per_col.sum()
        assert total > 0.0, name
        if c.kind == "cols":
            share = min(share, per_col[a:b].sum() / total)
        else:
            outside = np.r_[0:a, b:c.x.shape[1]]
            share = min(share, 1.0 - ((x64[:, outside] @ d64[outside]) ** 2).sum() / total)
        cond = max(cond, abs(loss32 / (total / (c.x.shape[0] * c.w.shape[1])) - 1.0))
    _conditions[name] = (float(share), float(cond))
    return _conditions[name]


def meets_conditions(name):
    share, cond = conditions(name)
    bar = SHARE_COLS if spotlight(name).kind == "cols" else 1.0
    return share >= bar and cond <= CONDITIONING, (name, share, cond)


# ---- plain random inputs at the edges of the shapes: (T, K, N, qtype, strategy, g); seed = 100 + position
PLAIN_SHAPES = [(1, 32, 7, "uint4", "group", 16), (3, 36, 5, "int4", "group", 4), (65, 77, 33, "int8", "channel", -1),
                (63, 48, 258, "uint4", "group", 8), (191, 64, 12, "uint4", "group", 32), (192, 64, 12, "uint4", "group", 32)]


def plain(i):
    t, k, n = PLAIN_SHAPES[i][:3]
    return inputs(100 + i, t, k, n)


# ---- a dead channel next to an outlier channel: the candidate scales stretch over five orders of magnitude
DEAD_OUTLIER_SHAPE = (96, 256, 64)
DEAD_OUTLIER_CONFIGS = [("uint4", "group", 32), ("int8", "channel", -1)]


def dead_outlier():
    if "dead" not in _cache:
        x, w = inputs(4, *DEAD_OUTLIER_SHAPE)
        x[:, 7] = 0.0
        x[:, 9] *= np.float32(1000.0)
        x.setflags(write=False)
        w.setflags(write=False)
        _cache["dead"] = (x, w)
    return _cache["dead"]


def dead_outlier_oracle(qtype, strategy, g):
    key = ("dead", qtype, strategy, g)
    if key not in _oracle:
        x, w = dead_outlier()
        _oracle[key] = O.awq_scale_search(x, w, qtype, strategy, g) + O.awq_clip_search(x, w, qtype, strategy, g)
    return _oracle[key]


# ---- K = 1100 input channels, int8 per channel: more than one lap of the 1024-thread and the 256-wide per-channel kernels
# T and N are this module's choice.  An RTN integer that sits on a tie flips when the candidate scale moves by an ulp, and the
# device's scales differ from the oracle's by a few ulp (powf, the order of the sums): the ORACLE's own loss moves by what one
# flipped integer is worth, 2 |x_k| step against a column's |X d_n| ~ sqrt(K / 12) |x| step, over N columns and sqrt(T) rows.  At
# 16 x 1100 x 24 a two-ulp change of the scales moves an oracle loss by 2.6e-3, more than the loss bar; at 48 x 1100 x 256 by
# 2.7e-4 (`scale_ulp_sensitivity`, checked in tests/test_awq_cases.py against a quarter of the bar).
WIDE_SHAPE = (48, 1100, 256)
WIDE_CONFIG = ("int8", "channel", -1)


def wide_channel_case():
    if "wide" not in _cache:
        x, w = inputs(1100, *WIDE_SHAPE)
        x.setflags(write=False)
        w.setflags(write=False)
        _cache["wide"] = (x, w)
    return _cache["wide"]


def scale_ulp_sensitivity(x, w, qtype, strategy, g, n_grid=20, ulps=2, trials=3):
    """Largest relative change of an oracle scale-search loss when every candidate scale moves `ulps` fp32 steps up or down."""
    ref_out = np.matmul(x, w)

    def losses(scales):
        out = []
        for scale in scales:
            col = scale.reshape(-1, 1)
            q, s, z = O.rtn_quantize(w * col, qtype, strategy, g)
            out.append(O._awq_loss(x, O.dequantize(q, s, z, rows_of=strategy, group_size=g) / col, ref_out))
        return np.array(out)

    base = candidate_scales(x, w, strategy, g, n_grid)
    l0, r, worst = losses(base), np.random.default_rng(0), 0.0
    for _ in range(trials):
        moved = base.copy()
        for _ in range(ulps):
            moved = np.nextafter(moved, np.where(r.random(base.shape) < 0.5, np.float32(np.inf), np.float32(0)).astype(np.float32))
        worst = max(worst, float(np.abs(losses(moved) / l0 - 1.0).max()))
    return worst
