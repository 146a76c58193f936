"""The exact HQQ tier without a GPU (tests/hqq_cases.py): the oracle and the restatement of the kernel's operation order give the
same bits on every case test_hqq_exact_gpu.py runs, so exactness is attainable; every such case meets the decision condition; and
the cases reach what they were chosen for.  A later GPU failure is localised by this file: GPU != both references -> the kernel
is wrong; the two references differ here -> the test is wrong."""
import numpy as np
import pytest

import hqq_cases as H
import oq_oracle as O
from conftest import load_json, synth_weight


@pytest.mark.parametrize("s", H.EXACT, ids=H.spec_id)
def test_kernel_order_reference_is_the_oracle_bit_for_bit(s):
    c = H.case(s)
    assert H.decisions_are_robust(c.trace), [e for e, _ in c.trace]
    best, trace = c.kernel_order()
    assert len(trace) == c.rounds
    for k, ((_, z_ref), (_, z_ora)) in enumerate(zip(trace, c.trace)):
        assert z_ref.tobytes() == z_ora.tobytes(), f"round {k}:\n" + H.describe_rows(z_ref, z_ora, c.kgroups)
    assert best.tobytes() == c.z.tobytes()
    assert np.isfinite(c.w).all() and np.isfinite(c.z).all()
    assert c.q.tobytes() == H.integers_given(c.w, c.s, c.z, s.group, c.p["reduce_range"]).tobytes()


@pytest.mark.parametrize("s, lp", H.ANY_NORM, ids=lambda v: H.spec_id(v) if isinstance(v, tuple) else str(v))
def test_the_restatement_follows_the_oracle_at_other_norms(s, lp):
    """np.exp2 / np.log2 stand in for the hardware's units there: close, not equal (the GPU is not equal either)."""
    c = H.case_at(s, lp)
    best, _ = c.kernel_order()
    assert np.abs(best - c.z).max() <= 2e-5


def test_tree_sum_is_numpy_s_pairwise_sum():
    r = np.random.default_rng(3)
    for n in (1, 4, 7, 8, 9, 12, 16, 20, 24, 40, 127, 128, 129, 136, 256, 264, 300, 520, 1031):
        v = (r.standard_normal((64, n)) * np.exp2(r.integers(-8, 8, (64, n)))).astype(np.float32)
        assert H.tree_sum(v).tobytes() == np.add.reduce(v, axis=1).tobytes(), n


def test_the_cases_reach_what_they_name():
    by = {H.spec_id(s): H.case(s) for s in H.EXACT}
    fixed = [c for c in by.values() if c.spec.params == "fixed"]
    mid = [c for c in by.values() if c.spec.params == "mid"]
    for cs in (fixed, mid):      # each on a register-tile group and on a general one
        assert {c.g in H.TILE_GROUPS for c in cs} == {True, False}
    for c in fixed:              # an early stop by a fixed point: the stopping round repeats the best round's zero points
        assert 1 < c.rounds < c.p["iters"] and c.trace[-1][1].tobytes() == c.trace[H.best_round(c.trace)][1].tobytes()
    for c in mid:                # `best` in the middle, with other bits than the last round: ctrl->pad / zp_best decide the result
        b = H.best_round(c.trace)
        assert 0 < b < c.rounds - 1 and c.rounds == c.p["iters"] and c.trace[b][1].tobytes() != c.trace[-1][1].tobytes()
        assert c.z.tobytes() == c.trace[b][1].tobytes()
    for c in by.values():
        if c.spec.params in ("i32", "i33", "nostop9"):
            assert c.rounds == c.p["iters"]
        if c.spec.kind == "ties":            # w / s + z0 on exact .5 ties, at even and odd levels
            t = c.rows / c.s + c.z0
            ties = (t - np.floor(t)) == 0.5
            assert ties.mean() > 0.5 and (np.floor(t[ties]) % 2 == 0).any() and (np.floor(t[ties]) % 2 == 1).any()
            assert (c.z0 == 8).all() and (np.log2(c.s) % 1 == 0).all()
        if c.spec.kind == "abi_div":         # ties of x / s + z that x * (1 / s) + z misses, towards either neighbour
            assert c.rounds == 1 and c.z.tobytes() == c.z0.tobytes()
            t = c.rows / c.s + c.z0
            other = np.clip(np.round(c.rows * (np.float32(1) / c.s) + c.z0), 0, 15)
            moved = other - np.clip(np.round(t), 0, 15)
            assert ((t - np.floor(t)) == 0.5).mean() > 0.9 and (moved > 0).sum() > 100 and (moved < 0).sum() > 100
        if c.spec.kind == "constant":
            assert (c.rows == c.rows[:, :1]).all()
    plain = H.case(H.spec(64, 257))
    for name in ("mse", "clip", "rr"):       # other initial parameters than the plain ones
        assert H.case(H.spec(64, 257, params=name)).s.tobytes() != plain.s.tobytes()
    sizes = {c.g for c in by.values()}
    assert sizes >= set(H.TILE_GROUPS) | set(H.GENERAL_GROUPS) | {96, 256}
    assert max(c.k * c.n for c in by.values()) <= 1600 * 520


def test_routes():
    assert H.routes(H.spec(64, 37)) == (False, True) and H.routes(H.spec(24, 37)) == (False,)
    assert H.routes(H.spec(256, 37)) == (False,) and H.routes(H.spec(256, 37, dtype="float16")) == (False, True)
    assert H.routes(H.spec(64, 37, params="i32")) == (False, True) and H.routes(H.spec(64, 37, params="i33")) == (False,)


def test_decision_condition():
    z = [np.full((2, 1), v, np.float32) for v in (1.0, 2.0, 3.0)]
    assert H.decisions_are_robust([(1.0, z[0]), (0.9, z[1]), (0.95, z[2])])
    assert not H.decisions_are_robust([(1.0, z[0]), (0.9, z[1]), (0.9 * (1 + 5e-6), z[2])])        # too close to the best error
    assert H.decisions_are_robust([(1.0, z[0]), (0.9, z[1]), (0.9, z[1].copy())])                  # ... unless it is a fixed point
    assert not H.decisions_are_robust([(1.0, z[0]), (0.9, z[1]), (0.95, z[2]), (0.9, z[0])])       # the bits of `best`, not of any round


def test_golden_c4_meets_the_decision_condition():
    """tests/golden/hqq.json::c4 has lp_norm = 1: test_hqq.py::test_gpu_matches_golden compares it byte for byte."""
    c4 = next(c for c in load_json("hqq.json")["cases"] if c["key"] == "c4")
    assert c4["lp_norm"] == 1.0
    w = synth_weight(c4["kind"], c4["seed"], c4["k"], c4["n"])
    rows = O.to_rows(w, "group", c4["group_size"])
    s, z0 = O.qparams_from_rows(rows, "uint4", "group", False, c4["reduce_range"], c4["clip_ratio"], c4["mse"], np.float32, np.float32)
    trace = []
    z = O.hqq_optimize_zero_point(rows, s, z0, c4["reduce_range"], 1.0, c4["beta"], c4["kappa"], c4["iters"], c4["early_stop"], trace=trace)
    assert H.decisions_are_robust(trace), [e for e, _ in trace]
    best, _ = H.kernel_order_reference(rows, s, z0, c4["reduce_range"], 1.0, c4["beta"], c4["kappa"], c4["iters"], c4["early_stop"])
    assert best.tobytes() == z.tobytes()
