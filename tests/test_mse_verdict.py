"""CPU-only checks of tests/mse_verdict.py, the judge of the MSE range search on the GPU: on synthetic error tables it must tell
decided rows from undecided ones, find the stop, and reject a planted wrong candidate on a decided row."""
import numpy as np
import pytest

import mse_verdict as V
import oq_oracle as O


def synthetic(e64, tau=1e-5):
    """Tables around a float64 error table [20, R]: candidate i has scale 1 - i/100, zero point 0, no subnormal terms."""
    e64 = np.asarray(e64, np.float64)
    r = e64.shape[1]
    scales = np.repeat((1 - np.arange(20) / 100.0).astype(np.float32)[:, None], r, axis=1)
    t = V.Tables(e64.astype(np.float32), e64, np.zeros((20, r), np.int64), np.full((20, r), 8, np.int64), 3.0, 8, scales,
                 np.zeros((20, r), np.int64), np.zeros(r, bool), "group", 8 * r)
    t.tau = tau
    return t


def walk(best_at, r=4):
    """Every row falls clearly until `best_at`, then rises clearly."""
    i = np.arange(20, dtype=np.float64)[:, None]
    return 1.0 + 0.05 * np.abs(i - best_at) + np.zeros((20, r))


def test_clear_rows_are_decided_and_near_ties_are_not():
    e = walk(7)
    e[8, 1] = e[7, 1] * (1 + 1e-5)          # row 1: candidate 8 within 2 tau of the best
    e[3, 2] = e[7, 2] * (1 - 1.5e-5)        # row 2: candidate 3 ahead of candidate 7 by less than 2 tau
    j = V.judge(synthetic(e))
    assert j.decided.tolist() == [True, False, False, True]
    assert j.winner.tolist() == [7, 7, 3, 7]
    # nothing improves at 9 .. 13; whether row 1 improves at 8 is inside the band, so the stop is 12 or 13
    assert j.stop == 12 and not j.stop_decided and j.stops == [12, 13]
    assert j.status[:8] == [1] * 8 and j.status[8] == -1 and not any(j.status[9:])


def test_stop_rule_counts_stale_iterations_globally_and_never_resets():
    e = walk(2)
    e[10:, 3] = np.linspace(0.9, 0.5, 10)    # row 3 starts improving again at iteration 10, too late: 3..7 were stale
    j = V.judge(synthetic(e))
    assert j.stop == 7 and j.stop_decided and j.winner.tolist() == [2, 2, 2, 2]
    e = walk(2)
    e[5, 3] = 0.5                            # one row improves at 5: stale iterations are 3, 4, 6, 7, 8
    j = V.judge(synthetic(e))
    assert j.stop == 8 and j.winner[3] == 5


def test_an_unclear_iteration_leaves_the_stop_undecided():
    e = walk(2)
    e[5, 0] = e[2, 0] * (1 - 1e-6)           # improves by far less than the band: stale or not is anyone's call
    j = V.judge(synthetic(e))
    assert not j.stop_decided and j.stops == [7, 8]
    assert not j.decided[0] and j.decided[1:].all()


def test_repeated_parameters_are_one_candidate():
    e = np.zeros((20, 3))                    # all-zero groups: twenty identical candidates, error 0 everywhere
    t = synthetic(e)
    t.scales[:] = 1.0
    j = V.judge(t)
    assert j.decided.all() and j.winner.tolist() == [0, 0, 0] and j.stop == 5 and j.stop_decided


def test_a_planted_wrong_candidate_on_a_decided_row_is_rejected():
    t = synthetic(walk(7))
    j = V.judge(t)
    s_ref, z_ref = t.scales[7].copy(), t.zps[7].copy()
    V.verdict(t, j, s_ref, z_ref, s_ref, z_ref)
    s_bad = s_ref.copy()
    s_bad[2] = t.scales[8, 2]                # the neighbouring candidate, 5 % worse
    with pytest.raises(AssertionError, match="decided rows differ"):
        V.verdict(t, j, s_bad, z_ref, s_ref, z_ref)


def test_undecided_rows_may_swap_inside_the_band_only():
    e = walk(7)
    e[8, 1] = e[7, 1] * (1 + 1e-5)
    t = synthetic(e)
    j = V.judge(t)
    s_ref, z_ref = t.scales[7].copy(), t.zps[7].copy()
    s_swap = s_ref.copy()
    s_swap[1] = t.scales[8, 1]
    v = V.verdict(t, j, s_swap, z_ref, s_ref, z_ref)
    assert (v.rows, v.undecided, v.differing) == (4, 1, 1)
    s_far = s_ref.copy()
    s_far[1] = t.scales[9, 1]
    with pytest.raises(AssertionError, match="outside the band"):
        V.verdict(t, j, s_far, z_ref, s_ref, z_ref)
    s_off = s_ref.copy()
    s_off[1] = np.float32(0.123)
    with pytest.raises(AssertionError, match="outside the candidate grid"):
        V.verdict(t, j, s_off, z_ref, s_ref, z_ref)


def test_the_band_is_derived_and_capped():
    assert V.tau_sum("group", 128, 0) == 127 * 2.0 ** -24
    assert V.tau_sum("tensor", 0, 1_202_300) == (4 + 6 + 2 + 1023) * 2.0 ** -24
    assert 8e-6 < V.tau_pow(30.0) < 1.2e-5
    w = np.random.default_rng(0).standard_normal((4096, 4), dtype=np.float32)
    assert V.tables(w, "uint4", "channel", -1, False, False).tau == V.CAP


def test_tables_are_the_oracles_and_the_oracle_sits_on_their_winner():
    w = np.random.default_rng(1).standard_normal((128, 64), dtype=np.float32)
    t = V.tables(w, "uint4", "group", 16, False, False)
    stop = V.oracle_stop(w, "uint4", "group", 16, False, False, t)      # asserts E32 == the oracle's trace bit for bit
    j = V.judge(t)
    assert j.stop == stop and 5 < stop < 19
    _, s, z = O.rtn_quantize(w, "uint4", "group", 16, False, False, 1.0, True)
    v = V.verdict(t, j, s, z, s, z)
    assert v.differing == 0 and v.undecided <= v.rows // 100


def test_underflowed_rows_keep_candidate_zero():
    w = (np.random.default_rng(5).standard_normal((128, 8), dtype=np.float32) * np.float32(1e-22)).astype(np.float32)
    t = V.tables(w, "uint4", "group", 128, False, False)
    j = V.judge(t)
    assert not t.e32.any() and j.absolute.all() and j.decided.all() and not j.winner.any() and j.stop == 5
