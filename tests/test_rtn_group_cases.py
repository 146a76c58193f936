"""The CPU side of tests/test_rtn_group_exact_gpu.py: what makes its cases tests is checked here on NumPy and the oracle alone,
so a machine without a GPU sees a case lose its point -- a generator change that leaves the rounding boundaries, a shape that no
longer reaches the build or the arm of the block map it is there for.  The restated map is held to being a map at all."""
import numpy as np
import pytest

import oq_oracle as O
import rtn_group_cases as R

ALL_BOUNDARY = R.BOUNDARY + R.EDGES


@pytest.mark.parametrize("case", ALL_BOUNDARY, ids=[c.id for c in ALL_BOUNDARY])
def test_boundary_dense_conditions_hold_on_the_oracle(case):
    """At least 1 % of the elements differ between rint(x * fl(1/s)) and the oracle, in the two-rounding form of the fused kernel and
    in the one-rounding form of the five-wave builds (a condition on the inputs; measured 3 % and more), no element is an exact tie
    of either form (a residual of 0.5 fires the redo whatever the band is), every level the grid can reach occurs, and every row
    of every strip of the build holds an element that differs in both forms: every ballot has to fire because of the band, and
    every redo has to be right."""
    w, (q, s, z) = R.boundary_input(case.id)
    c = R.conditions(w, case.g, *case.grid, lpr=case.lpr)
    print(f"{case.id}: {case.k} x {case.n} g {case.g} {case.build}: naive_share {c['naive_share']:.4f}, fma form {c['fma_share']:.4f}, exact ties "
          f"{c['exact_ties']}, least used level {c['least_level'][0]} x {c['least_level'][1]} of {c['levels']} levels, strip rows {c['strip_rows']:.4f}")
    assert c["naive_share"] >= R.NAIVE_SHARE and c["fma_share"] >= R.NAIVE_SHARE, c
    assert c["exact_ties"] == 0.0, c
    assert c["least_level"][1] >= 1, c
    assert c["strip_rows"] == 1.0, c
    assert np.isfinite(w).all() and np.isfinite(s).all()
    if case.huge:      # scale >= 1e30: `make_colq` sets thr = -1, next to ordinary groups in the same lanes
        kg = case.k // case.g
        big = s.reshape(case.n, kg) >= 1e30
        assert sorted(zip(*map(list, np.nonzero(big.T)))) == sorted(case.huge)
    if case.seed == 0 and not case.huge:      # the second matrix of the list / batch tests
        w2, _ = R.boundary_input(case.id, 1)
        assert not np.array_equal(w, w2)


@pytest.mark.parametrize("case", ALL_BOUNDARY, ids=[c.id for c in ALL_BOUNDARY])
def test_every_case_takes_the_build_its_comment_names(case):
    assert R.build_of(case.k, case.n, case.g, case.bits, case.layout, case.emit_q) == case.build
    if case.layout == "nbits" and case.g in R.WAVE_GROUPS:
        p = R.wave_plan(case.k, case.n, case.g, case.bits)
        assert p["ncol_tiles"] >= 2 or case in R.EDGES
        assert case.k // case.g in (2, 3)


def test_the_edge_cases_are_the_edges_they_name():
    live = {c.n: (R.wave_plan(c.k, c.n, c.g, 4)["ncol_tiles"], R.wave_plan(c.k, c.n, c.g, 4)["live_strips_of_last_tile"]) for c in R.EDGES}
    assert live == {4: (1, 1), 36: (1, 2), 100: (1, 4), 124: (1, 4), 132: (2, 1)}
    assert all(R.wave_plan(c.k, c.n, c.g, 4)["build"] == "pair" for c in R.EDGES)
    assert all(R.wave_plan(k, n, 128, 4)["build"] == "pair" for k, n in R.STORE_SHAPES)
    assert all(R.BOUNDARY_BY_ID[name].build in ("pair", "wave<16,5>") for name, _ in R.LISTS)


@pytest.mark.parametrize("k,n,g,build,xg,arms,live", R.ORDERS, ids=[f"{o[0]}x{o[1]}-g{o[2]}" for o in R.ORDERS])
def test_the_restated_block_map_is_a_bijection_and_takes_the_arms(k, n, g, build, xg, arms, live):
    p = R.wave_plan(k, n, g, 4)
    print(f"{k} x {n} g {g}: {p['build']}, {p['nrow_tiles']} x {p['ncol_tiles']} tiles, xg_log2 {p['xg_log2']}, arms {sorted(p['arms'])}")
    assert (p["build"], p["xg_log2"], p["arms"], p["live_strips_of_last_tile"]) == (build, xg, arms, live)
    want = {(r, c) for r in range(p["nrow_tiles"]) for c in range(p["ncol_tiles"])}
    assert len(p["tiles"]) == len(want) and set(p["tiles"]) == want
    assert p["nrow_tiles"] > p["gk"] and p["nrow_tiles"] % p["gk"] != 0          # a full band followed by a short one


def test_the_block_map_is_a_bijection_on_every_small_grid():
    """Every (row tiles, column tiles, xg_log2) up to 11 x 70: the restatement of `tile_of_block` visits every tile once."""
    for g, bits in ((128, 4), (128, 8), (64, 4), (32, 4)):
        for kgroups in range(1, 12):
            for n in (4, 132, 1028, 2180, 2304, 4100, 8192, 8964):
                p = R.wave_plan(kgroups * g, n, g, bits)
                want = {(r, c) for r in range(p["nrow_tiles"]) for c in range(p["ncol_tiles"])}
                assert len(p["tiles"]) == len(want) and set(p["tiles"]) == want, (g, bits, kgroups, n)


def test_iid_normal_weights_never_reach_the_boundaries():
    """Why the boundary-dense inputs exist: on the weights the existing tests use, the two formulas agree everywhere."""
    w, _ = R.normal_input(1024, 256, 128)
    c = R.conditions(w, 128, "uint4")
    print(f"i.i.d. normal 1024 x 256: naive_share {c['naive_share']}")
    assert c["naive_share"] < 1e-4


def test_where_wrong_names_the_cell_the_lane_set_and_the_element():
    want = np.zeros((256, 256), np.uint8)
    got = want.copy()
    got[128 + 35, 128 + 70] = 3          # k-group 1, column tile 1, strip 2, lane set 2, lane column 1, slot 2
    msg = R.where_wrong(got, want, 256, 256, 128, lpr=8)
    assert "1 of 65536" in msg and "(1, 1, 2): 1" in msg and "per lane set: 2: 1" in msg
    assert "row 163 (k-group 1, row 35 of it), column 198 (lane column 1, slot 2): got 3, oracle 0" in msg
    assert R.where_wrong(want, want, 256, 256, 128) == ""
    s = np.ones((256, 2), np.float32)
    t = s.copy()
    t[7, 1] = np.nextafter(np.float32(1), np.float32(2))
    assert "first at column 7, k-group 1" in R.where_params_wrong(t, s, 256, 2, "scale") and R.where_params_wrong(s, s, 256, 2, "scale") == ""


def test_the_layout_helpers_invert_the_oracles_packers():
    q = np.random.default_rng(3).integers(-8, 8, (256, 12)).astype(np.int8)
    u = R.unsigned_levels(q, 4)
    blob = O.matmul_nbits_layout(u, np.ones((24, 1), np.float32), np.zeros((24, 1), np.uint8), 128, 4)[0]
    np.testing.assert_array_equal(R.blob_to_kn(blob, 256, 12, 128, 4), u)
    np.testing.assert_array_equal(R.packed4_to_kn(O.pack_nibbles(q), 256, 12), u)
    q8 = np.random.default_rng(4).integers(0, 256, (64, 8)).astype(np.uint8)
    blob8 = O.matmul_nbits_layout(q8, np.ones((16, 1), np.float32), np.zeros((16, 1), np.uint8), 32, 8)[0]
    np.testing.assert_array_equal(R.blob_to_kn(blob8, 64, 8, 32, 8), q8)
