"""The CPU side of tests/test_awq_edges_gpu.py: what makes its spotlight cases tests is checked here on the oracle alone, so a
machine without a GPU sees a case lose its point (a seed or recipe change that spreads the loss, a candidate whose fp32 loss is
mostly cancellation).  The helpers of tests/awq_cases.py that restate the oracle's loop are tied to the oracle bit for bit."""
import numpy as np
import pytest

import awq_cases as A
import oq_oracle as O


@pytest.mark.parametrize("name", list(A.SPOTLIGHTS))
def test_spotlight_conditions_hold_on_the_oracle(name):
    """Region share >= 0.999 (columns) or exactly 1 (rows), and |oracle fp32 loss / float64 loss - 1| <= 2e-4 for each of the
    20 + 10 candidates.  Measured: shares >= 0.99954 (C2) and 1.0; conditioning <= 1.3e-5."""
    c = A.spotlight(name)
    share, cond = A.conditions(name)
    print(f"{name}: least region share {share!r}, fp32 vs float64 {cond:.2e}")
    if c.kind == "cols":
        assert share >= A.SHARE_COLS, (name, share)
    else:
        assert share == 1.0, (name, share)
        a, b = c.region
        assert not c.x[:, :a].any() and not c.x[:, b:].any()
        assert (O.awq_activation_scale(c.x)[a:b] > 0).all()
    assert cond <= A.CONDITIONING, (name, cond)
    assert A.meets_conditions(name)[0]
    es, el, er, ecl = A.oracle(name)
    assert np.isfinite(es).all() and np.isfinite(el).all() and np.isfinite(ecl).all() and el.min() > 0 and ecl.min() > 0


@pytest.mark.parametrize("name", ["C1", "C3", "R1", "R5"])
def test_a_column_spotlight_leaves_the_weight_statistic_alone_and_tiling_leaves_the_losses(name):
    c = A.spotlight(name)
    if c.kind == "cols":
        plain = A.inputs(A.SPOTLIGHTS[name][1], *A.SPOTLIGHTS[name][2:5])[1]
        np.testing.assert_allclose(O.awq_weight_scale(c.w, c.strategy, c.g), O.awq_weight_scale(plain, c.strategy, c.g), rtol=1e-6)
    tiled = A.tiled_for_gram(c.x, c.x.shape[1])
    assert tiled.shape[0] >= 3 * c.x.shape[1] and tiled.shape[0] % c.x.shape[0] == 0
    _, el, _, ecl = A.oracle(name)
    _, tl = O.awq_scale_search(tiled, c.w, c.qtype, c.strategy, c.g, c.sym)
    np.testing.assert_allclose(tl, el, rtol=2e-4)                       # the same mean over repeated rows: a tenth of the loss bar
    np.testing.assert_allclose(O.awq_activation_scale(tiled), O.awq_activation_scale(c.x), rtol=1e-6)


@pytest.mark.parametrize("n_grid", [1, 7, 20])
def test_the_restated_candidates_are_the_oracles(n_grid):
    """`candidate_scales` and `scale_residuals` against O.awq_scale_search: the winner's row bit for bit, and every loss from
    W - D (which is W^ up to one fp32 rounding of W, 6e-8 |w| against |d| >= |w| / 300 or so: 1e-4 on the loss is generous)."""
    c = A.spotlight("C3")
    es, el = O.awq_scale_search(c.x, c.w, c.qtype, c.strategy, c.g, c.sym, n_grid=n_grid)
    cand = A.candidate_scales(c.x, c.w, c.strategy, c.g, n_grid)
    assert cand.shape == (n_grid, c.x.shape[1])
    np.testing.assert_array_equal(cand[int(np.argmin(el))], es)
    ds = A.scale_residuals(c.x, c.w, c.qtype, c.strategy, c.g, c.sym, n_grid=n_grid)
    ref_out = np.matmul(c.x, c.w)
    for d, loss in zip(ds, el):
        assert O._awq_loss(c.x, c.w - d, ref_out) == pytest.approx(loss, rel=1e-4)


def test_the_wide_case_is_not_decided_by_one_flipped_integer():
    """48 x 1100 x 256, int8 per channel: a two-ulp change of every candidate scale (what separates the device's scales from the
    oracle's) moves the oracle's own losses by at most a quarter of the 2e-3 loss bar.  Measured 2.7e-4; 2.6e-3 at 16 x 1100 x 24."""
    x, w = A.wide_channel_case()
    moved = A.scale_ulp_sensitivity(x, w, *A.WIDE_CONFIG)
    print(f"wide case: largest loss change under a two-ulp change of the scales {moved:.2e}")
    assert moved <= 5e-4, moved
    assert A.scale_ulp_sensitivity(*A.inputs(1100, 16, 1100, 24), *A.WIDE_CONFIG) > 2e-3          # the shape that could not hold the bar
