"""The recipes and restatements of tests/gptq_factor_cases.py, checked on the host: the cases the GPU file uses are exact by
`exact_ok`'s own count, the closed forms are what they claim, the widths reach every launch kind of `factor_batched`, and `locate`
names the launch of a wrong element."""
import numpy as np
import pytest

import gptq_factor_cases as F

PIVOT_K = 388
PIVOTS = (0, 31, 32, 127, 128, 384, 387)
BATCHED = ((388, 3), (640, 3), (1536, 2))


def gpu_cases():
    """(K, keyword arguments of `width_case`, method, count) of every exact factor call of tests/test_gptq_factor_exact_gpu.py;
    the matrices are built when a test asks"""
    out = []
    for K in F.WIDTHS:
        for method in F.methods_of(K):
            out.append((K, {}, method, 1))
    for K in F.DAMPED:
        out.append((K, dict(damped=True), "auto", 1))
    out.append((PIVOT_K, dict(dead=(100,)), "auto", 1))
    for K, count in BATCHED:
        for m in range(count):
            out.append((K, dict(seed=10 + m), "auto", count))
    return out


@pytest.mark.parametrize("K,kw,method,count", gpu_cases(), ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_exact_ok(K, kw, method, count):
    """every partial sum of every product of the chain is an fp32 number, every operand of a piece leg its own first piece, and the
    restated chain arrives at the closed form"""
    case = F.width_case(K, **kw)
    r = F.exact_ok(case, method, count)
    assert r.units < F.LIMIT, (r.units, r.worst)
    assert r.piece_bits <= 11
    has_pieces = any(l.get("leg") == "pieces" for l in F.legs(case.K, count, method))
    assert (r.piece_bits > 0) == has_pieces
    assert np.array_equal(r.x, case.linv)


@pytest.mark.parametrize("K", F.WIDTHS)
def test_closed_form(K):
    for case in [F.width_case(K)] + ([F.width_case(K, damped=True)] if K in F.DAMPED else []):
        l, linv = case.l, case.linv
        assert np.array_equal(l, np.rint(l)) and np.array_equal(4 * linv, np.rint(4 * linv))
        assert float((np.abs(4 * linv) @ np.abs(l)).max()) < 2.0 ** 53       # integers in float64: the product is exact
        assert np.array_equal((4 * linv) @ l, 4 * np.eye(K))
        assert np.array_equal(np.triu(case.u), case.u) and np.array_equal(case.u.astype(np.float64), linv[::-1, ::-1])
        p = F.reversed_p(case)
        assert np.array_equal(p, l @ l.T) and np.array_equal(p, p.T)
        h64 = p[::-1, ::-1] - case.damp * np.eye(K)
        assert np.array_equal(case.h.astype(np.float64), h64), "H is not its own fp32 rounding"
        assert np.abs(case.u).max() <= 128 and np.abs(case.h).max() < 1 << 15


@pytest.mark.parametrize("K", F.DAMPED)
def test_damp_identity(K):
    """damp_kernel: d = fl32(percdamp * fl32(t / K)) with t the exact fp32 sum of the diagonal"""
    case = F.width_case(K, damped=True)
    assert case.damp in F.DAMPS and case.percdamp > 0
    diag = np.diagonal(case.h).astype(np.float64)
    assert np.abs(diag).sum() * 8 < F.LIMIT and np.array_equal(diag * 8, np.rint(diag * 8))
    t = np.float32(diag.sum())
    assert float(t) == diag.sum()
    p = np.float32(case.percdamp)
    assert float(p) == case.percdamp
    assert np.float32(p * np.float32(t / np.float32(K))) == np.float32(case.damp)
    assert np.array_equal(np.diagonal(case.h) + np.float32(case.damp), np.diagonal(F.reversed_p(case))[::-1].astype(np.float32))


def test_dead_case():
    case = F.width_case(PIVOT_K, dead=(100,))
    j = PIVOT_K - 1 - 100
    assert case.h[100, 100] == 0.0 and not case.h[100].any() and not case.h[:, 100].any()
    assert case.l[j, j] == 1.0 and np.count_nonzero(case.l[j]) == 1 and np.count_nonzero(case.l[:, j]) == 1
    assert case.u[100, 100] == 1.0


@pytest.mark.parametrize("kind", ("zero", "negative", "nan"))
@pytest.mark.parametrize("j", PIVOTS)
def test_pivot_case(j, kind):
    """the leading minors in front of j are untouched, minor j + 1 is not positive definite, the diagonal sum stays finite for j > 0"""
    base = F.width_case(PIVOT_K)
    case = F.pivot_case(base, j, kind)
    assert case.info == j + 1 and np.array_equal(case.u, np.eye(PIVOT_K, dtype=np.float32))
    p, p0 = F.reversed_p(case), F.reversed_p(base)
    assert np.array_equal(p[:j, :j], p0[:j, :j])
    if kind == "nan":
        assert np.isnan(p[j, max(j - 1, 0)]) and (j == 0 or np.isfinite(np.diagonal(p)).all())
    else:
        pivot = p[j, j] - (base.l[j, :j] ** 2).sum()
        assert pivot == 0 if kind == "zero" else pivot < 0


# ------------------------------------------------------------------------------------ the widths reach every launch kind
def all_legs():
    return [(K, m, l) for K in F.WIDTHS for m in F.methods_of(K) for l in F.legs(K, 1, m)]


def test_legs_restate_the_table():
    """the legs each width of the GPU file is the smallest to reach"""
    def of(K, kind, method="auto", **kw):
        return [l for l in F.legs(K, 1, method) if l["kind"] == kind and all(l[k] == v for k, v in kw.items())]
    for K in (1, 33, 96, 128):
        assert F.legs(K) == [dict(kind="diag", kb=0, n=K)]
    assert of(129, "panel")[0] | dict(kb=0) == dict(kind="panel", kb=0, M=128, N=1, Kd=128, arm_a="vector", arm_b="scalar")
    assert of(129, "strip", M=1, N=1, arm_a="scalar", arm_b="scalar") and of(129, "level", b=128, shape="ragged", b2=1)
    assert all(l[a] == "vector" for l in F.legs(256) for a in l if a.startswith("arm_"))
    assert of(256, "level") == of(256, "level", shape="full", pairs=1, b2=128) and len(of(256, "level")) == 1
    assert of(388, "diag", n=4) and of(388, "level", b=128, shape="full", pairs=1) and of(388, "level", b=128, shape="ragged", first=1, b2=4)
    assert of(388, "level", b=256, shape="ragged", b2=132)
    assert all(l[a] == "vector" for l in F.legs(388) for a in l if a.startswith("arm_"))
    assert of(515, "deferred", leg="gemm_tn", n=3, tiles=1, arm_a="scalar") and of(515, "strip", arm_a="scalar", arm_b="scalar")
    assert of(515, "panel", arm_b="scalar") and of(515, "level", arm_a1="scalar", arm_b1="scalar", arm_a2="scalar", arm_b2="vector")
    assert of(640, "deferred", leg="gemm_tn", n=128, tiles=1, padded=False)
    assert of(640, "level", b=128) == of(640, "level", b=128, shape="full", pairs=2)          # block 4 stays alone at b = 128
    assert of(640, "level", b=512, shape="ragged", b2=128)
    assert [l["n"] for l in of(1100, "deferred")] == [588, 76] and of(1100, "deferred", n=588, tiles=5, upper_tiles=15, padded=True)
    assert [(l["leg"], l["n"]) for l in of(1536, "deferred")] == [("pieces", 1024), ("gemm_tn", 512)]
    assert of(1536, "deferred", leg="pieces", padded=False)
    assert of(1536, "deferred", "f32", leg="gemm_tn", n=1024, tiles=8, super_tiles=1)
    assert of(1664, "deferred", "f32", leg="gemm_tn", n=1152, tiles=9, super_tiles=2) and of(1664, "deferred", leg="pieces", n=1152, padded=True)
    assert not any(l.get("leg") == "pieces" for K in F.WIDTHS for l in F.legs(K, 1, "f32"))
    assert of(2176, "level", leg="pieces") == of(2176, "level", b=2048, shape="ragged", b2=128, pairs=1) and of(2176, "level", leg="pieces")
    assert of(4096, "level", leg="pieces") == of(4096, "level", b=2048, shape="full", pairs=1) and of(4096, "level", leg="pieces")
    assert of(2176, "level", "f32", b=2048, leg="gemm_tn") and of(4096, "level", "f32", b=2048, leg="gemm_tn")
    assert not any(l["kind"] == "level" and l["leg"] == "pieces" for K in F.WIDTHS if K < 2176 for l in F.legs(K))


def test_legs_cover_every_kind():
    seen = all_legs()
    diag_n = {l["n"] for _, _, l in seen if l["kind"] == "diag"}
    assert {1, 33, 96, 128} <= diag_n and any(n % 4 for n in diag_n) and any(n < 128 and n % 4 == 0 for n in diag_n)
    for kind in ("panel", "strip"):
        arms = {(l["arm_a"], l["arm_b"]) for _, _, l in seen if l["kind"] == kind}
        assert ("vector", "vector") in arms and any(b == "scalar" for _, b in arms), (kind, arms)
    assert ("scalar", "scalar") in {(l["arm_a"], l["arm_b"]) for _, _, l in seen if l["kind"] == "strip"}
    assert any(l["kind"] == "strip" and l["M"] == 384 for _, _, l in seen) and any(l["kind"] == "strip" and l["M"] == 1 for _, _, l in seen)
    deferred = [(m, l) for _, m, l in seen if l["kind"] == "deferred"]
    assert {(l["leg"], l["padded"]) for _, l in deferred} == {("gemm_tn", False), ("gemm_tn", True), ("pieces", False), ("pieces", True)}
    assert {1, 2} <= {l["super_tiles"] for _, l in deferred if l["leg"] == "gemm_tn"}
    assert {"vector", "scalar"} <= {l["arm_a"] for _, l in deferred if l["leg"] == "gemm_tn"}
    assert any(l["leg"] == "gemm_tn" and l["tiles"] > 1 and l["padded"] for _, l in deferred)     # mirror stores with a ragged edge
    levels = [l for _, _, l in seen if l["kind"] == "level"]
    assert {(l["leg"], l["shape"]) for l in levels} == {(a, b) for a in ("gemm_tn", "pieces") for b in ("full", "ragged")}
    assert any(l["pairs"] > 1 for l in levels) and {1, 4, 128, 132} <= {l["b2"] for l in levels if l["shape"] == "ragged"}
    assert any(l["first"] > 0 for l in levels)
    assert {128, 256, 512, 1024, 2048} == {l["b"] for l in levels}
    for arm in ("arm_a1", "arm_b1", "arm_a2"):
        assert {"vector", "scalar"} <= {l[arm] for l in levels if l["leg"] == "gemm_tn"}
    # the same level at b = 2048 runs on either leg, by the method alone
    assert {m for K, m, l in seen if l["kind"] == "level" and l["b"] == 2048 and l["leg"] == "gemm_tn"} == {"f32"}


def test_legs_batched():
    """a batch changes no shape; its strides between matrices are multiples of four floats, so no arm changes either"""
    for K, count in BATCHED:
        assert F.legs(K, count, "auto") == F.legs(K, 1, "auto")
    assert F.pieces_ok(1536, 2, "auto") and not F.pieces_ok(1536, 2, "f32")


# ------------------------------------------------------------------------------------ locate
def test_locate_names_the_leg():
    """one element of the expected U flipped in the region of each launch that writes X (a mutation of the numpy side only)"""
    K = 388
    u = F.width_case(K).u

    def at(r, c):       # position of X -> what `locate` says about a U wrong there
        got = u.copy()
        got[K - 1 - r, K - 1 - c] += 1.0
        found = F.locate(K, got != u)
        assert sum(found.values()) == 1
        return next(iter(found))

    assert at(5, 3) == "diag block 0, sub-block 0"
    assert at(127, 127) == "diag block 0, sub-block 3"
    assert at(140, 130) == "diag block 1, sub-block 0"
    assert at(128 + 70, 128 + 2) == "diag block 1, off-diagonal phase row 2"
    assert at(387, 384) == "diag block 3, sub-block 0"
    assert at(128, 0) == "level 128, full pair 0, tile (0, 0)"
    assert at(255, 127) == "level 128, full pair 0, tile (0, 0)"
    assert at(384, 256) == "level 128, ragged pair 1, tile (0, 0)"
    assert at(387, 383) == "level 128, ragged pair 1, tile (0, 0)"
    assert at(256, 0) == "level 256, ragged pair 0, tile (0, 0)"
    assert at(300, 200) == "level 256, ragged pair 0, tile (0, 1)"
    assert at(387, 255) == "level 256, ragged pair 0, tile (1, 1)"
    assert at(3, 5) == "zero triangle (finish_factor_kernel)"
    # every launch that writes X owns some element, and `describe` counts them
    names = set()
    for r in range(0, K, 16):
        for c in range(0, r + 1, 16):
            names.add(at(r, c))
    for leg in F.legs(K):
        if leg["kind"] == "diag":
            assert any(n.startswith(f"diag block {leg['kb']},") for n in names)
        if leg["kind"] == "level":
            for p in range(leg["first"], leg["first"] + leg["pairs"]):
                assert any(n.startswith(f"level {leg['b']}, {leg['shape']} pair {p},") for n in names), leg
    xw = np.zeros((K, K), dtype=bool)
    xw[256:384, 0:128] = True
    wrong = xw[::-1, ::-1]
    assert F.describe(K, wrong) == "level 256, ragged pair 0, tile (0, 0): 16384 wrong"
    assert F.describe(K, np.zeros((K, K), dtype=bool)) == "nothing wrong"


def test_locate_large():
    K = 4096
    wrong = np.zeros((K, K), dtype=bool)
    wrong[K - 1 - 2048, K - 1 - 2047] = True
    wrong[K - 1 - 4095, K - 1 - 0] = True
    assert F.locate(K, wrong) == {"level 2048, full pair 0, tile (0, 15)": 1, "level 2048, full pair 0, tile (15, 0)": 1}
    K = 2176
    wrong = np.zeros((K, K), dtype=bool)
    wrong[K - 1 - 2100, K - 1 - 300] = True
    assert F.locate(K, wrong) == {"level 2048, ragged pair 0, tile (0, 2)": 1}
