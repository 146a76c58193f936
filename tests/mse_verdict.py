"""Row-by-row parity verdict for the MSE range search (utils.py:140-239, `csrc/rtn_mse.hip`).  An ordinary module, imported by
tests/test_mse_gpu.py and (CPU only) tests/test_mse_verdict.py.

NumPy's float32 `power` and its pairwise sums cannot be reproduced bit for bit on the GPU, so two candidates of a row whose errors
differ in the last bits may swap.  This module decides, from the reference's arithmetic alone, WHICH rows that may happen to, and
holds every other row to bit equality.  Nothing in it is fitted to what the kernel returns.

Tables of a case (`Tables`), all 20 candidates, from the oracle's own steps (`O.to_rows`, `O.min_max`, `O.qparams`, `O.fake_quantize`):
  d    per-element difference fake_quantize(x) - x, float32, exactly the reference's;
  E32  sum(power(|d|, 2.4)) in float32 with NumPy's own kernels: the reference's table (checked against `O.min_max_mse(trace=)`);
  E64  sum(|d|.astype(float64) ** 2.4): the plain high-precision value of the same formula.

The band `tau` of a case = min(tau_sum + tau_pow + tau_numpy, 1e-4)  (1e-4 is the bound the suite had before; it is never exceeded)
  tau_sum   first-order bound of the kernel's summation order, u = 2^-24, non-negative terms:
            * channel / group (`mse_rows_kernel`: `err += fake_quant_error(...)`, and `mse_rows_reg_kernel`: `err += e[r]`):
              one sequential accumulator over the m elements of the row                                        -> (m - 1) u
            * tensor: `mse_tensor_partial` `acc[i] += ...` over c = ceil(K N / 262144) elements per thread      -> (c - 1) u
                      `v += __shfl_xor(v, off, 64)`, six butterfly levels                                       -> 6 u
                      `(s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3])`                                           -> 2 u
                      `mse_tensor_mask` `err += partial[b * kMseSteps + i]` over 1024 partials                  -> 1023 u
  tau_pow   `exp2(2.4f * log2 |d|)` with v_log_f32 and v_exp_f32 at their documented 1 ulp: the logarithm L carries a relative
            2^-23, the product 2.4f * L a rounding of 2^-24, and the constant 2.4f differs from 2.4 by 3.97e-8 relative, so the
            exponent is off by at most 2.4 |L| (2^-23 + 2^-24 + 3.97e-8) and the result by ln 2 times that, plus 2^-23 for the
            exponential itself.  |L| is taken as max |log2 |d|| over the elements with d != 0 of the whole case.
  tau_numpy max |E32 / E64 - 1| over the entries whose E32 is a normal finite number (the others fall under the absolute rule),
            measured on the CPU from the reference's arithmetic.

Two candidates with the same (scale bits, zero point) are one candidate: they give the same d, hence the same sum on either side.

Rows.  S = the stop iteration; candidates 0..S were executed.
  relative rule (every executed E32 of the row is zero or a normal finite number): with b the first minimum of E64[0..S], the row is
      DECIDED when every other executed candidate i has E64[i] > E64[b] (1 + 2 tau) + a[i] + a[b], where a = n_sub * 2^-149 and
      n_sub counts the entry's terms below 2^-126: the reference rounds each of those to the subnormal grid, which may move it by
      one subnormal ulp against any other evaluation.
  absolute rule (some executed E32 of the row is subnormal or inf; `tau` is meaningless): the row is decided by E32 ordering alone,
      when every other executed candidate lies more than 4 subnormal ulps (2 per entry) above the first minimum of E32.  An entry
      none of whose terms reaches 2^-151 is exactly zero in every evaluation and gets no margin: among such entries the earlier
      candidate keeps the row, as `err < best` is strict (utils.py:225).  The rule also takes the rows whose E32 underflowed.  An `inf`
      entry never improves (it loses against FLT_MAX, utils.py:190) and counts as clearly `inf` when E64 > FLT_MAX (1 + 1e-4).
      Why "4": sums of subnormal terms are exact, so two evaluations differ only where a term's own rounding to the subnormal grid
      flips; with a power accurate to ~1e-6 that happens to well under one term per row, and 4 leaves room for two flips per entry.
  A DECIDED row must equal the oracle bit for bit: scale, zero point, every integer.  An UNDECIDED row must end on a candidate of
  the grid at or before the stop whose error is within the same margin of the best (and within 1e-4 in E32, the previous rule).
  Rows holding a NaN have NaN errors, never improve and keep candidate 0; they are compared with the oracle directly.

The stop.  Iteration i "improves" when some row's error is below that row's running minimum (utils.py:225).  With the margins above an
iteration is clearly improving (some row improves by more than the margin), clearly stale (every row misses by more than the margin,
or repeats the parameters of its running minimum), or unclear.  The stop is DECIDED when no iteration up to it is unclear; it then
must equal the oracle's.  If it is not, every stop that the unclear iterations allow is considered and a row is decided only when it
has the same clear winner under all of them.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

import oq_oracle as O

CAP = 1e-4
U = 2.0 ** -24
SUB = 2.0 ** -149
TINY = 2.0 ** -126
FLT_MAX = float(np.finfo(np.float32).max)
TENSOR_THREADS = 1024 * 256        # mse_tensor_partial: 1024 blocks of 256 threads
TENSOR_PARTIALS = 1024
C24_ERR = abs(float(np.float32(2.4)) / 2.4 - 1.0)
ABS_ULPS = 4


def rows_of(w, strategy, g):
    return np.ascontiguousarray(w).reshape(1, -1) if strategy == "tensor" else np.ascontiguousarray(O.to_rows(w, strategy, g))


@dataclass
class Tables:
    e32: np.ndarray            # [20, R] float32, the reference's table (all 20 candidates)
    e64: np.ndarray            # [20, R] float64
    n_sub: np.ndarray          # [20, R] terms below 2^-126
    n_live: np.ndarray         # [20, R] terms of at least 2^-151 (anything smaller rounds to zero in every evaluation)
    max_l: float               # max |log2 |d|| over contributing elements
    m: int                     # elements per row
    scales: np.ndarray         # [20, R] float32
    zps: np.ndarray            # [20, R]
    nan_rows: np.ndarray       # [R] bool
    strategy: str
    total: int                 # elements of the tensor
    tau: float = 0.0
    parts: dict = field(default_factory=dict)


def tau_sum(strategy: str, m: int, total: int) -> float:
    if strategy == "tensor":
        per_thread = -(-total // TENSOR_THREADS)
        return (max(per_thread - 1, 0) + 6 + 2 + (TENSOR_PARTIALS - 1)) * U
    return (m - 1) * U


def tau_pow(max_l: float) -> float:
    return math.log(2.0) * 2.4 * max_l * (2.0 ** -23 + 2.0 ** -24 + C24_ERR) + 2.0 ** -23


def tables(w, qtype, strategy, g, sym, red) -> Tables:
    """All 20 candidates of the search on `w` [K, N]: the reference's float32 table, the float64 one and what the band needs."""
    ref_rows = O.to_rows(w, strategy, g)                      # the layout the reference sums over (2-D for the tensor strategy)
    lo0, hi0 = O.min_max(ref_rows, strategy, 1.0)
    tensor = strategy == "tensor"
    nrows = 1 if tensor else ref_rows.shape[0]
    e32 = np.empty((O.MSE_STEPS, nrows), np.float32)
    e64 = np.empty((O.MSE_STEPS, nrows), np.float64)
    n_sub = np.zeros((O.MSE_STEPS, nrows), np.int64)
    n_live = np.zeros((O.MSE_STEPS, nrows), np.int64)
    scales = np.empty((O.MSE_STEPS, nrows), np.float32)
    zps = np.empty((O.MSE_STEPS, nrows), np.int64)
    max_l = 0.0
    with np.errstate(all="ignore"):
        for i in range(O.MSE_STEPS):
            p = 1 - i / O.MSE_GRID
            s, z = O.qparams(p * lo0, p * hi0, qtype, sym, red)
            d = O.fake_quantize(ref_rows, s, z, qtype, sym, red)
            d -= ref_rows
            a = np.abs(d)
            t32 = np.power(a, O.MSE_NORM)
            e32[i] = np.reshape(np.sum(t32) if tensor else np.sum(t32, axis=1), -1)
            t64 = a.astype(np.float64) ** 2.4
            e64[i] = np.reshape(np.sum(t64) if tensor else np.sum(t64, axis=1), -1)
            sub = (t64 > 0) & (t64 < TINY)
            n_sub[i] = np.reshape(np.sum(sub) if tensor else np.sum(sub, axis=1), -1)
            big = t64 >= SUB / 4
            n_live[i] = np.reshape(np.sum(big) if tensor else np.sum(big, axis=1), -1)
            live = np.isfinite(a) & (a >= TINY)               # a subnormal |d| contributes 0 on either side
            if live.any():
                max_l = max(max_l, float(np.max(np.abs(np.log2(a[live].astype(np.float64))))))
            scales[i] = np.reshape(s, -1)
            zps[i] = np.reshape(z, -1)
    nan_rows = np.isnan(e32).any(axis=0)
    m = ref_rows.size if tensor else ref_rows.shape[1]
    t = Tables(e32, e64, n_sub, n_live, max_l, m, scales, zps, nan_rows, strategy, int(np.size(w)))
    ok = np.isfinite(e64) & np.isfinite(e32) & (e32 >= TINY)
    t_np = float(np.max(np.abs(e32[ok].astype(np.float64) / e64[ok] - 1.0))) if ok.any() else 0.0
    t.parts = dict(tau_sum=tau_sum(strategy, m, t.total), tau_pow=tau_pow(max_l), tau_numpy=t_np)
    t.tau = min(sum(t.parts.values()), CAP)
    return t


def oracle_stop(w, qtype, strategy, g, sym, red, t: Tables | None = None) -> int:
    """Last iteration the oracle executed; with `t`, also checks that the oracle's own trace is `t.e32` bit for bit."""
    trace = []
    O.min_max_mse(O.to_rows(w, strategy, g), qtype, strategy, sym, red, trace=trace)
    if t is not None:
        for i, e in trace:
            assert np.asarray(e, np.float32).reshape(-1).tobytes() == t.e32[i].tobytes(), f"iteration {i}: not the oracle's table"
    return len(trace) - 1


@dataclass
class Judgement:
    stop: int                  # the reference's stop (from the tables)
    stop_decided: bool
    stops: list                # every stop the unclear iterations allow
    winner: np.ndarray         # [R] first minimum among 0..stop (reference arithmetic, E32 ordering for the absolute rule)
    decided: np.ndarray        # [R] bool
    absolute: np.ndarray       # [R] bool: judged by the absolute rule
    tau: float
    status: list = field(default_factory=list)   # per iteration: +1 clearly improving, 0 clearly stale, -1 unclear


def _same_params(t: Tables, i, j):
    """Per row: do candidates i[row] and j[row] carry the same (scale bits, zero point)?"""
    cols = np.arange(t.e32.shape[1])
    return (t.scales[i, cols].view(np.uint32) == t.scales[j, cols].view(np.uint32)) & (t.zps[i, cols] == t.zps[j, cols])


def stop_from_flags(flags) -> int:
    """utils.py:232-237: the fifth iteration in which nothing improved is the last one executed."""
    stale_n = 0
    for i, f in enumerate(flags):
        stale_n += 0 if f else 1
        if stale_n >= O.MSE_PATIENCE:
            return i
    return O.MSE_STEPS - 1


def _absolute_rows(t: Tables, last: int):
    e = t.e32[: last + 1]
    return (np.isinf(e) | ((e < TINY) & (t.e64[: last + 1] > 0))).any(axis=0) & ~t.nan_rows


def _keys(t: Tables, absolute):
    """Per row the table that orders its candidates and the (relative, absolute) margins of one comparison."""
    e32 = t.e32.astype(np.float64)
    clearly_inf = np.isinf(t.e32) & (t.e64 > FLT_MAX * (1 + CAP))
    vague_inf = np.isinf(t.e32) & ~clearly_inf
    key = np.where(absolute[None, :], e32, t.e64)
    key = np.where(np.isinf(t.e32) & absolute[None, :], np.inf, key)
    rel = np.where(absolute, 0.0, 2 * t.tau)
    ab = np.where(absolute[None, :], np.minimum(ABS_ULPS / 2, t.n_live) * SUB, t.n_sub * SUB)
    return key, rel, ab, vague_inf


def judge(t: Tables, stop: int | None = None) -> Judgement:
    """`stop`: the stop of a larger matrix these rows are a part of (the rule is global), taken as decided."""
    forced = stop
    r = t.e32.shape[1]
    absolute = _absolute_rows(t, O.MSE_STEPS - 1)
    key, rel, ab, vague_inf = _keys(t, absolute)
    cols = np.arange(r)
    # ---- the stop: walk the iterations, each row against its running minimum
    run = np.full(r, FLT_MAX)                # running minimum (reference ordering: first strict improvement wins)
    run_i = np.zeros(r, int)                 # its candidate; best_min/max start as candidate 0 (utils.py:191-192)
    status = []                              # per iteration: +1 clearly improving, 0 clearly stale, -1 unclear
    with np.errstate(all="ignore"):
        for i in range(O.MSE_STEPS):
            k = key[i]
            margin = ab[i] + np.where(run < FLT_MAX, ab[run_i, cols], 0.0)
            improves = k * (1 + rel) + margin < run
            repeats = _same_params(t, np.full(r, i), run_i) & (run < FLT_MAX)
            exact = (margin == 0) & (rel == 0)            # both sums are the same number in every evaluation (all terms vanish)
            stale = (k > run * (1 + rel) + margin) | (exact & (k >= run)) | repeats | t.nan_rows | (np.isinf(k) & ~vague_inf[i])
            improves &= ~t.nan_rows & ~vague_inf[i] & ~repeats
            status.append(1 if improves.any() else (0 if stale.all() else -1))
            better = (k < run) & ~t.nan_rows
            run = np.where(better, k, run)
            run_i = np.where(better, i, run_i)

    stop_of = stop_from_flags

    # the reference's own stop, from its own float32 table
    ref_run = np.full(r, np.float32(FLT_MAX))
    ref_flags = []
    with np.errstate(all="ignore"):
        for i in range(O.MSE_STEPS):
            b = t.e32[i] < ref_run
            ref_flags.append(bool(b.any()))
            ref_run = np.where(b, t.e32[i], ref_run)
    stop = stop_of(ref_flags)
    if forced is not None:
        stop, stops, stop_decided = forced, [forced], True
    elif all(s >= 0 for s in status[: stop + 1]):
        assert [s == 1 for s in status[: stop + 1]] == ref_flags[: stop + 1], "clear iterations disagree with the reference's table"
        stops, stop_decided = [stop], True
    else:                                    # unclear iterations read as stale give the earliest stop, as improving the latest
        lo = stop_of([s == 1 for s in status])
        hi = stop_of([s != 0 for s in status])
        stops, stop_decided = list(range(min(lo, stop), max(hi, stop) + 1)), False
    # ---- rows: the same clear winner under every allowed stop
    decided = np.ones(r, bool)
    winner0 = None
    with np.errstate(all="ignore"):
        for s_last in stops:
            k = key[: s_last + 1].copy()
            k[np.isnan(k)] = np.inf
            k[0] = np.where(np.isinf(k).all(axis=0), 0.0, k[0])          # nothing ever improves: candidate 0 stays
            win = np.argmin(k, axis=0)
            kb = k[win, cols]
            clear = np.ones(r, bool)
            for i in range(s_last + 1):
                rival = ~_same_params(t, np.full(r, i), win)
                margin = ab[i] + ab[win, cols]
                exact = (margin == 0) & (rel == 0) & (i > win)          # an exact tie: the earlier candidate keeps the row
                clear &= ~rival | (k[i] > kb * (1 + rel) + margin) | (exact & (k[i] >= kb))
            clear &= ~vague_inf[: s_last + 1].any(axis=0)
            decided &= clear
            if winner0 is None:
                winner0 = win
            decided &= win == winner0
            if s_last == stop:
                winner = win
    decided &= ~t.nan_rows
    return Judgement(stop, stop_decided, stops, winner, decided, absolute, t.tau, status)


@dataclass
class Verdict:
    rows: int
    undecided: int
    differing: int
    nan_rows: int
    stop: int
    stop_decided: bool
    tau: float

    def as_properties(self):
        return dict(rows=self.rows, undecided=self.undecided, differing=self.differing, stop=self.stop,
                    stop_decided=self.stop_decided, tau=self.tau)


def verdict(t: Tables, j: Judgement, s_gpu, z_gpu, s_ref, z_ref, q_gpu_rows=None, q_ref_rows=None, what="", requantize=None) -> Verdict:
    """Judge one result.  `s_*`, `z_*` flat per-row parameters (GPU and oracle), `q_*_rows` [R, m] integers or None.
    `requantize(row, scale, zp)` -> the reference's integers of that row under those parameters: the integers of an undecided row
    that ended on another candidate are held to the candidate the GPU chose."""
    r = t.e32.shape[1]
    sg = np.ascontiguousarray(s_gpu, np.float32).reshape(-1)
    so = np.ascontiguousarray(s_ref, np.float32).reshape(-1)
    zg, zo = np.asarray(z_gpu).reshape(-1).astype(np.int64), np.asarray(z_ref).reshape(-1).astype(np.int64)
    assert sg.size == r and so.size == r
    cols = np.arange(r)
    same = (sg.view(np.uint32) == so.view(np.uint32)) & (zg == zo)
    nan = t.nan_rows
    assert np.all(np.isnan(sg[nan]) == np.isnan(so[nan])) and np.all(zg[nan] == zo[nan]), f"{what}: NaN rows differ from the oracle"
    same |= nan & np.isnan(sg) & np.isnan(so) & (zg == zo)
    # the oracle itself must sit on the winner of its own table wherever the row is decided (a helper / oracle consistency check)
    ow = j.winner
    on_winner = (t.scales[ow, cols].view(np.uint32) == so.view(np.uint32)) & (t.zps[ow, cols] == zo)
    assert np.all(on_winner[j.decided]), f"{what}: the oracle is off its own table on a decided row"
    bad = j.decided & ~same
    assert not bad.any(), (f"{what}: {int(bad.sum())} decided rows differ from the oracle (first: row {int(np.flatnonzero(bad)[0])}, "
                           f"tau {t.tau:.3g}, stop {j.stop})")
    # undecided rows: on the grid, at or before the last allowed stop, within the margin of the best
    last = max(j.stops)
    und = ~j.decided & ~nan
    key, rel, ab, _ = _keys(t, j.absolute)
    for row in np.flatnonzero(und & ~same):
        hits = [i for i in range(last + 1)
                if t.scales[i, row].view(np.uint32) == sg[row:row + 1].view(np.uint32)[0] and t.zps[i, row] == zg[row]]
        assert hits, f"{what}: row {row} ended on a range outside the candidate grid (or after the stop {last})"
        i = hits[0]
        with np.errstate(all="ignore"):
            k = key[: last + 1, row].copy()
            k[np.isnan(k)] = np.inf
            b = int(np.argmin(k))
            assert k[i] <= k[b] * (1 + rel[row]) + ab[i, row] + ab[b, row], f"{what}: undecided row {row} is outside the band"
            e = t.e32[: last + 1, row].astype(np.float64)
            assert e[i] <= np.nanmin(e) * (1 + CAP) + ABS_ULPS * SUB, f"{what}: undecided row {row} misses the 1e-4 rule"
        if q_gpu_rows is not None and requantize is not None:
            np.testing.assert_array_equal(q_gpu_rows[row], np.reshape(requantize(row, t.scales[i, row], t.zps[i, row]), -1),
                                          err_msg=f"{what}: integers of undecided row {row} are not those of its own candidate {i}")
    if q_gpu_rows is not None:
        ok = same & ~nan
        np.testing.assert_array_equal(q_gpu_rows[ok], q_ref_rows[ok], err_msg=f"{what}: integers of rows on the oracle's candidate")
    return Verdict(r, int(und.sum()), int((~same).sum()), int(nan.sum()), j.stop, j.stop_decided, t.tau)
