"""The case list of test_gptq_loop_exact_gpu.py, checked on the host (tests/gptq_loop_cases.py): every exact case satisfies the
conditions under which `oq_gptq_loop_f32` owes the float64 loop's bytes, the planted parameters come out of the oracle's own
`qparams`, no weight clamps that was not meant to, the parameter-version probes separate a stale read from a fresh one, and the list
reaches every kernel, specialisation and update leg of csrc/gptq_loop.hip.  No library call."""
import numpy as np
import pytest

import oq_oracle as O
import gptq_loop_cases as G


@pytest.mark.parametrize("name", list(G.CASES))
def test_the_case_is_exact_planted_and_unclamped(name):
    c, res = G.restated(name)
    assert G.exact_ok(c, res), (res.exact, res.mass_units)
    assert res.mass_units <= 2.0 ** 16                                        # far below the 2^24 the argument needs
    qmin, qmax = O.qrange(c.qtype, c.symmetric, c.reduce_range)
    if c.g:
        assert np.array_equal(res.used_scale, c.planted), "a group's scale is not the planted power of two"
        mant, _ = np.frexp(res.used_scale)
        assert (mant == 0.5).all()
        assert res.used_zp.min() >= qmin and res.used_zp.max() <= qmax
        # both ends of the grid occur in every column: the low byte of the magic-number sum at qmin and qmax
        assert ((res.q == qmin).any(axis=0) & (res.q == qmax).any(axis=0)).all()
    free = ~(c.anchors | c.clamps)
    assert not ((res.q[free] == qmin) | (res.q[free] == qmax)).any(), "a row clamps that was not planted to"
    if c.clamps.any():
        assert ((res.q[c.clamps] == qmin) | (res.q[c.clamps] == qmax)).all()
    # ties at the half level occur, on both sides of the zero point's parity
    y = c.w[free].astype(np.float64) / (c.scale if len(c.init_scale) > 1 or c.g else 1.0)
    assert (np.abs(y - np.floor(y) - 0.5) == 0).any() or c.w.shape[0] < 3
    # every error is on the column's unit grid
    for _, e in res.err:
        assert np.array_equal(e / c.unit, np.round(e / c.unit))


def test_odd_and_even_zero_points_meet_ties():
    """Round-half-even of w / s must not depend on the zero point's parity: the list holds ties under odd and under even ones."""
    seen = set()
    for name in ("one-128x64-groups", "type-uint8", "type-int4"):
        c, res = G.restated(name)
        free = ~(c.anchors | c.clamps)
        y = c.w.astype(np.float64) / c.scale
        tie = (np.abs(y - np.floor(y)) == 0.5) & free[:, None]
        z = np.broadcast_to(res.used_zp[0], tie.shape)
        seen |= {int(v) & 1 for v in z[tie]}
    assert seen == {0, 1}


@pytest.mark.parametrize("name", G.VERSION_CASES)
def test_the_version_probes_yield_both_scales(name):
    c, res = G.restated(name)
    want = G.expected_versions(c)
    assert set(want.values()) == {1, 2}, want
    for tgt, f in want.items():
        assert np.array_equal(res.used_scale[tgt], f * c.scale), (tgt, f)
        # the other reading of the rows would have given the other scale: the probe moved the maximum by the grid's span
    rt = G.routes(*c.w.shape, c.g, c.block_size)
    kinds = set()
    for i, tgt in c.versions:
        start = tgt * c.g
        la_i = [l for l in rt["launches"] if l["i1"] <= i < l["i1"] + l["count"]][0]
        la_t = [l for l in rt["launches"] if l["i1"] <= start < l["i1"] + l["count"]][0]
        kinds.add("same launch" if la_i is la_t else "same block" if i // c.block_size == start // c.block_size
                  else "same super-block" if i // rt["S"] == start // rt["S"] else "earlier super-block")
    if rt["tall"]:
        assert {"same launch", "same block", "earlier super-block"} <= kinds, kinds          # a tall block is its own super-block
    else:
        assert {"same launch", "same super-block"} <= kinds, kinds
    if name == "versions-1100-128-128":
        assert kinds == {"same launch", "same super-block", "earlier super-block"}


def all_routes(mode):
    return {name: G.routes(*shape, mode) for name, shape in G.SHAPES.items()}


def test_the_case_list_reaches_every_route():
    rts = all_routes("corrected")
    launches = [la for rt in rts.values() for la in rt["launches"]]
    assert {la["kernel"] for la in launches} == {"rows16", "block"}
    assert {la["kernel"] for rt in all_routes("corrected_columns").values() for la in rt["launches"]} == {"block"}
    slabs = {s for la in launches for s in la["slabs"]}
    assert slabs == {f"live{n}" for n in range(8)} | {"ragged"}, sorted(slabs)
    updates = [la["update"] for la in launches if la["update"]]
    assert ("panel", ()) in updates
    reasons = {w for kind, why in updates if kind == "gemm_tn" for w in why}
    assert reasons == {"M % 4", "N % 4", "lda % 4", "A unaligned"}, reasons
    assert {("gemm_tn", (w,)) for w in reasons} <= set(updates)                             # each of them also as the only reason
    legs = {d["leg"] for rt in rts.values() for d in rt["deferred"]}
    assert legs == {"pieces", "gemm_tn"}
    assert [d["leg"] for d in rts["deferred-1536x1024"]["deferred"]] == ["pieces", "gemm_tn"]
    assert all(d["leg"] == "gemm_tn" for d in G.routes(1536, 1024, 128, 128, method="f32")["deferred"])
    assert {rt["tall"] for rt in rts.values()} == {True, False}
    S = {n: (rt["S"], G.SHAPES[n][3], G.SHAPES[n][2]) for n, rt in rts.items() if not rt["tall"]}
    assert any(s == 512 for s, _, _ in S.values())
    assert any(s < 512 and s > bs and g and s % g == 0 for s, bs, g in S.values()), "no S below 512 from an lcm"
    assert any(s == bs and g and G._lcm(bs, g) > 512 for s, bs, g in S.values()), "no S = block_size from an lcm above 512"
    # a tall block whose last launch is short, and a ragged last super-block
    assert any(rt["tall"] and any(la["count"] == 64 and not la["block_start"] for la in rt["launches"]) for rt in rts.values())
    assert any(not rt["tall"] and rt["launches"][-1]["count"] % 16 for rt in rts.values())


def test_the_dense_cases_fill_both_coefficient_planes():
    """Every (source slab, target slab) pair of a 128-row rows16 launch carries a nonzero coefficient somewhere: m = target - source
    is the slot of the coefficient image, plane A for m < 4 and plane B above."""
    pairs = set()
    for name in ("one-128x63", "one-128x64-groups"):
        c = G.CASES[name]()
        rt = G.routes(*c.w.shape, c.g, c.block_size)
        assert [la["kernel"] for la in rt["launches"]] == ["rows16"]
        i, j = np.nonzero(np.triu(c.u, 1))
        pairs |= set(zip((i // 16).tolist(), (j // 16).tolist()))
    assert pairs == {(a, b) for a in range(8) for b in range(a, 8)}
    assert {b - a for a, b in pairs} == set(range(8))
    # and in the multi-launch cases both planes are live inside a launch, next to the panel update's and the deferred product's operands
    c = G.CASES["multi-256-128-128-64"]()
    i, j = np.nonzero(np.triu(c.u, 1))
    same = i // 128 == j // 128
    assert ((j[same] // 16 - i[same] // 16) >= 4).any() and ((j[same] // 16 - i[same] // 16) < 4).any() and (~same).any()


def test_routes_restates_the_documented_examples():
    rt = G.routes(640, 132, 48, 128)
    assert rt["S"] == 384 and [la["i1"] for la in rt["launches"]] == [0, 128, 256, 384, 512]
    rt = G.routes(700, 52, 1024, 128)
    assert rt["S"] == 128 and all(la["update"] is None for la in rt["launches"]) and len(rt["deferred"]) == 5
    rt = G.routes(640, 130, 64, 320)
    assert rt["tall"] and [(la["ord"], la["i1"], la["count"]) for la in rt["launches"]] == [(0, 0, 128), (1, 128, 128), (2, 256, 64), (3, 320, 128),
                                                                                         (4, 448, 128), (5, 576, 64)]
    rt = G.routes(300, 52, 24, 128)
    assert {la["kernel"] for la in rt["launches"]} == {"block"}
    rt = G.routes(520, 64, 0, 24)
    assert {la["kernel"] for la in rt["launches"]} == {"block"} and rt["S"] == 504
    rt = G.routes(200, 130, 16, 64)
    assert rt["S"] == 512 and rt["launches"][-1]["slabs"] == ["ragged"] and rt["launches"][-1]["count"] == 8


def test_locate_names_the_launch_slab_and_lane():
    wrong = np.zeros((640, 130), dtype=bool)
    wrong[128 + 37, 6] = True                     # launch 1, slab 2, r16 5, c4 2
    wrong[320:, 9] = True
    hits, follows = G.locate(wrong, 640, 130, 64, 320)
    assert dict(ord=1, kernel="rows16", i1=128, slab=2, r16=5, c4=2, count=1) in hits
    assert follows == {"inside a slab": 1, "a super-block boundary": 1}
    text = G.describe(wrong, 640, 130, 64, 320)
    assert "321 wrong" in text and "rows16" in text and "super-block boundary" in text
    assert G.describe(np.zeros((4, 4), dtype=bool), 4, 4, 0, 128) == "no mismatch"


def test_the_fp32_family_adds_exact_zeros_outside_a_launch():
    for K, N, g, bs in G.FP32_SHAPES:
        w, u, s, z = G.fp32_case(K, N, g, bs)
        rt = G.routes(K, N, g, bs)
        inside = np.zeros((K, K), dtype=bool)
        for la in rt["launches"]:
            inside[la["i1"]:la["i1"] + la["count"], la["i1"]:la["i1"] + la["count"]] = True
        assert not u[~inside].any() and np.array_equal(u, np.triu(u))
        res = G.restate(w, u, "uint8", g, bs, False, False, s, z, dtype=np.float32)
        assert res.q_deq.dtype == np.float32 and np.isfinite(res.q_deq).all()
        assert np.abs(w).min() > 2.0 ** -100 and np.abs(w).max() < 2.0 ** 100
        if g:                                     # the parameters in force are the oracle's, on the rows as the reference finds them
            lo, hi = O.min_max(res.w[:g].T, "channel")
            ps, pz = O.qparams(lo, hi, "uint8", False, False)
            assert np.array_equal(res.used_scale[0], ps.reshape(-1)) and np.array_equal(res.used_zp[0], pz.reshape(-1))


def test_the_contraction_case_separates_fused_from_rounded_products():
    w, u, s, z, targets = G.contraction_case()
    K, N = w.shape
    assert [la["kernel"] for la in G.routes(K, N, 0, 128)["launches"]] == ["rows16"]
    res = G.restate(w, u, "uint8", 0, 128, False, False, s, z, dtype=np.float32)
    assert (res.q[~targets] == z).all() and (res.q[targets] == z).all()                  # 1/2 rounds to the even level: the zero point
    # the same update with the product left unrounded: every target lands above the half
    i, j = np.nonzero(np.triu(u, 1))
    assert np.array_equal(np.sort(j), np.flatnonzero(targets)) and set((j // 16 - i // 16).tolist()) == set(range(1, 8))
    e = w[i].astype(np.float64) / 0.25
    fused = (w[j].astype(np.float64) - u[i, j].astype(np.float64)[:, None] * e).astype(np.float32)
    assert (fused == np.float32(0.5) + np.float32(2.0 ** -24)).all()
    assert (np.round(fused) == 1).all()
