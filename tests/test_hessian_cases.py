"""hessian_cases.py checked on the CPU: every case test_hessian_exact_gpu.py compares on bits satisfies `exact_ok`, the recipes tell
the methods apart, `slices_of` gives the slice counts the GPU file claims, `locate` names a planted element, and the restated
splits are lossless and round as torch does."""
import numpy as np
import pytest
import torch

import hessian_cases as hc


def test_every_gpu_case_is_exact():
    """All elements under bf16x6 and f16x3 and on small integers; under f32 and bf16x9 (`three_pieces_apart`) every off-diagonal
    element, and every diagonal one of a column without a three-piece entry: x^2 of an 18-bit x is no fp32 number.  Prints the
    largest mass per (method, recipe), in units, and what the mask leaves out."""
    largest, left_out = {}, {}
    for method, recipe, T, K, n_seen, n_add in hc.exact_cases():
        x = hc.RECIPES[recipe](T, K)
        h0 = hc.integer_h0(x, K) if n_seen else None
        ex = hc.exact_ok(method, x, n_seen, n_add, h0)
        case = (method, recipe, T, K, n_seen, n_add)
        assert ex.lossless, case
        key = (method, recipe)
        largest[key] = max(largest.get(key, 0.0), float(ex.units[ex.mask].max(initial=0.0)))
        if method in hc.KEEPS_EVERYTHING and recipe == "three_pieces_apart":
            off = ~ex.mask & ~np.eye(K, dtype=bool)
            assert not off.any(), case
            lo = hc.split_bf16x3(x)[2]
            assert not (~np.diag(ex.mask) & ~(lo != 0).any(axis=0)).any(), case       # only columns with a live lo piece
            left_out[key] = max(left_out.get(key, 0), int((~ex.mask).sum()))
        else:
            assert ex.all, (case, int((~ex.mask).sum()), float(ex.units.max()))
        v = hc.kept_sum(method, x, n_seen + n_add)
        assert (v != 0).any()
    for key in sorted(largest):
        print(f"{key[0]:7s} {key[1]:20s} largest mass 2^{np.log2(max(largest[key], 1.0)):.2f} units, left to the bound: at most {left_out.get(key, 0)} elements")
        assert largest[key] < 2.0 ** 24


def test_the_wide_recipes_keep_their_pieces_live_in_every_chunk():
    for T, K in [(33, 40), (65, 40), (33, 260), (1009, 520), (1537, 300), (4096, 40)]:
        for p in hc.split_bf16x3(hc.three_pieces(T, K))[1:] + hc.split_bf16x3(hc.three_pieces_apart(T, K))[1:]:
            live = (p != 0).any(axis=1)
            assert all(live[c:c + 8].any() for c in range(0, T, 8)), (T, K)
        _, lo, _ = hc.split_f16x2_hessian(hc.two_pieces(T, K), 1.0)
        live = (lo != 0).any(axis=1)
        assert all(live[c:c + 8].any() for c in range(0, T, 8)), (T, K)


@pytest.mark.parametrize("T,K", [(33, 40), (33, 260), (1009, 520), (993, 520)])
def test_the_recipes_tell_the_methods_apart(T, K):
    """f32 (sx = 1) and bf16x9 keep every product: their kept sum IS the float64 product.  bf16x6 on `three_pieces` and f16x3 on
    `two_pieces` must differ from it, and from each other, on the diagonal and off it: otherwise a wrong term set would go unseen."""
    off = ~np.eye(K, dtype=bool)
    for method, recipe in (("bf16x6", "three_pieces"), ("f16x3", "two_pieces")):
        x = hc.RECIPES[recipe](T, K)
        true = x.astype(np.float64).T @ x.astype(np.float64)
        kept = {m: hc.kept_sum(m, x) for m in hc.METHODS}
        np.testing.assert_array_equal(kept["bf16x9"], true)
        np.testing.assert_array_equal(kept["f32"], true)
        for other in [true] + [kept[m] for m in hc.METHODS if m != method]:
            differs = kept[method] != other
            assert (differs & off).any() and np.diag(differs).any(), (method, recipe)
        assert hc.exact_ok(method, x).all
    # every single product of a term set matters: dropping any one changes the bits
    for method, recipe in (("bf16x6", "three_pieces"), ("bf16x9", "three_pieces"), ("f16x3", "two_pieces")):
        x = hc.RECIPES[recipe](T, K)
        pieces, div = hc.pieces_of(method, x, 2)
        full = hc.kept_sum(method, x)
        for p, q in hc.TERMS[method]:
            assert (pieces[p].T @ pieces[q]).any(), (method, recipe, p, q)
            assert (full - (pieces[p].T @ pieces[q]) / div != full).any()


def _expected_without(method, x, drop, n_seen=0, n_add=2, h0=None):
    """`expected` of a kernel that leaves the piece product `drop` out."""
    pieces, div = hc.pieces_of(method, x, n_seen + n_add)
    v = sum(pieces[p].T @ pieces[q] for p, q in hc.TERMS[method] if (p, q) != drop) / div
    return hc.epilogue(method, v, n_seen, n_add, h0)


def test_what_the_gpu_cases_of_bf16x9_can_and_cannot_tell():
    """On the recipes the GPU file RUNS under bf16x9 and on the elements it compares on bits:
    - a kernel that drops any one of hi.hi, hi.mid, mid.hi, mid.mid, hi.lo, lo.hi returns other bits (mid.mid only on `mid_pairs`,
      where two two-piece elements meet and the product is still an fp32 number; hi.lo and lo.hi on `three_pieces_apart`);
    - lo.lo, lo.mid and mid.lo cannot be shown by any order-independent fp32 result: an element with a live lo has at least 18
      significant bits and one with a live mid at least 9, so a product in which lo.mid is not zero has at least 26, and lo.lo 35.
      Where these products are live the sum is no fp32 number.  Hence `expected` of bf16x9 and of bf16x6 agree on every compared
      element: the suite cannot tell syrk_pieces_kernel<9> from <6>.  That is a finding about fp32 outputs, stated here so that
      it is not mistaken for coverage."""
    seen = {t: set() for t in hc.TERMS["bf16x9"]}
    for method, recipe, T, K, n_seen, n_add in hc.exact_cases():
        if method != "bf16x9" or K > 600 or (n_seen and T != 33):
            continue
        x = hc.RECIPES[recipe](T, K)
        h0 = hc.integer_h0(x, K) if n_seen else None
        mask = hc.exact_ok(method, x, n_seen, n_add, h0).mask
        want = hc.expected(method, x, n_seen, n_add, h0)
        for term in hc.TERMS["bf16x9"]:
            if ((want != _expected_without(method, x, term, n_seen, n_add, h0)) & mask).any():
                seen[term].add(recipe)
        assert np.array_equal(want[mask], hc.expected("bf16x6", x, n_seen, n_add, h0)[mask])
    for term in [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)]:
        assert seen[term], term
    assert seen[(1, 1)] == {"mid_pairs"} and "three_pieces_apart" in seen[(0, 2)] and "three_pieces_apart" in seen[(2, 0)]
    for term in [(2, 2), (2, 1), (1, 2)]:
        assert not seen[term], term
    # the same for the other piece methods: every product they keep shows in the bits of some GPU case
    for method in ("bf16x6", "f16x3"):
        shown = set()
        for m, recipe, T, K, n_seen, n_add in hc.exact_cases():
            if m != method or K > 300 or n_seen:
                continue
            x = hc.RECIPES[recipe](T, K)
            want = hc.expected(method, x)
            shown |= {t for t in hc.TERMS[method] if (want != _expected_without(method, x, t)).any()}
        assert shown == set(hc.TERMS[method]), (method, shown)


def test_slice_counts():
    """What the GPU file claims, for a workspace that never binds, for the pieces alone and for room for exactly two slabs."""
    for method, shapes in hc.SLICE_SHAPES.items():
        counts = set()
        for (T, K), want in shapes.items():
            s = hc.slices_of(method, T, K, hc.FULL)
            assert s.count == want, (method, T, K, s)
            counts.add(min(s.count, 3))
            assert (s.count - 1) * s.per + s.last == (T if method == "f32" else hc.ceil_div(T, hc.STAGE_ROWS[method]))
            assert 0 < s.last <= s.per
            # the budget the query of the library hands out is as good as unlimited: 16 slabs
            assert hc.slices_of(method, T, K, 16 * K * K * 4) == s
            none = hc.slices_of(method, T, K, hc.slab_bytes_in(method, T, K, 0 if method == "f32" else hc.pieces_workspace_bytes(T, K)))
            two_bytes = 2 * K * K * 4 if method == "f32" else hc.pieces_workspace_bytes(T, K, 2 * K * K * 4)
            two = hc.slices_of(method, T, K, hc.slab_bytes_in(method, T, K, two_bytes))
            assert hc.slab_bytes_in(method, T, K, two_bytes) == 2 * K * K * 4
            assert none.count == 1 and two.count == (1 if want == 1 or (method != "f32" and K == 300) else 2), (method, T, K, none, two)
            print(f"{method:7s} T={T:5d} K={K:4d}: {s.count:2d} slices of {s.per} (last {s.last}); pieces only {none.count}, two slabs {two.count}")
        assert counts == {1, 2, 3}, method
        assert any(hc.slices_of(method, T, K, hc.FULL).last < hc.slices_of(method, T, K, hc.FULL).per for (T, K), n in shapes.items() if n >= 2), method
        assert any(hc.slices_of(method, T, K, hc.FULL).last < hc.slices_of(method, T, K, hc.FULL).per for (T, K), n in shapes.items() if n >= 3), method
    # f32: the first split at 512 rows, none at 511; one tile, so ceil(4096 / tiles) never binds
    assert hc.first_split_rows("f32", 40) == 512 and hc.slices_of("f32", 511, 40, hc.FULL).count == 1
    # six tiles (K = 520): two slices as soon as both have 512 rows after padding to the stage -- 32 stages of 32, 64 of 16
    assert hc.first_split_rows("f16x3", 520) == 31 * 32 + 1 == 993
    assert hc.first_split_rows("bf16x6", 520) == hc.first_split_rows("bf16x9", 520) == 63 * 16 + 1 == 1009
    for method, first in (("f16x3", 993), ("bf16x6", 1009), ("bf16x9", 1009)):
        assert (first - 1, 520) in hc.SLICE_SHAPES[method] and (first, 520) in hc.SLICE_SHAPES[method]
    # three tiles (K = 300): two slices gain less than 0.02 of a round, three are the first split
    assert hc.first_split_rows("f16x3", 300) == 47 * 32 + 1 == 1505 and hc.slices_of("f16x3", 1505, 300, hc.FULL).count == 3
    assert hc.first_split_rows("bf16x6", 300) == 95 * 16 + 1 == 1521
    # one tile: the 0.02 rule wants seven slices at once
    assert hc.slices_of("f16x3", 2081, 40, hc.FULL).count == 1 and hc.slices_of("f16x3", 7 * 512, 40, hc.FULL).count == 7
    # the other shapes of the GPU file
    for method in hc.METHODS:
        for T, K in hc.RUNNING_SHAPES[method]:
            assert (hc.slices_of(method, T, K, hc.FULL).count > 1) == (T > 33)
    assert hc.slices_of("f16x3", 993, 520, 3 * 520 * 520 * 4).count == 2


def test_locate_names_a_planted_element():
    K = 600
    mask = np.zeros((K, K), dtype=bool)
    mask[70, 300] = True          # tile (0, 1) of 256: wave row 1, wave column 0; upper
    mask[300, 70] = True          # its mirror image
    mask[520, 520] = True         # tile (2, 2), diagonal
    got = hc.locate(mask, "f16x3", K)
    assert got == {hc.Place(0, 1, 1, 0, "upper", "vector"): 1, hc.Place(0, 1, 1, 0, "mirrored", "scalar"): 1,
                   hc.Place(2, 2, 0, 0, "diagonal", "vector"): 1}
    assert all(p.store == "scalar" for p in hc.locate(mask, "f16x3", K, sliced=True))
    assert all(p.store == "scalar" for p in hc.locate(mask, "f16x3", K, aligned=False))
    assert all(p.store == "scalar" for p in hc.locate(mask, "bf16x6", K))
    # f32: 128-tiles, waves of 32 rows at w * 32 and 64 + w * 32
    assert hc.locate(mask, "f32", K) == {hc.Place(0, 2, 0, 1, "upper", "scalar"): 1, hc.Place(0, 2, 0, 1, "mirrored", "scalar"): 1,
                                         hc.Place(4, 4, 0, 0, "diagonal", "scalar"): 1}
    # a diagonal tile's group of four that starts left of the diagonal is stored by scalars; K % 4 != 0 too
    m2 = np.zeros((260, 260), dtype=bool)
    m2[5, 6] = m2[5, 8] = m2[3, 258] = True
    places = hc.locate(m2, "f16x3", 260)
    assert places == {hc.Place(0, 0, 0, 0, "upper", "scalar"): 1, hc.Place(0, 0, 0, 0, "upper", "vector"): 1, hc.Place(0, 1, 0, 0, "upper", "vector"): 1}
    assert all(p.store == "scalar" for p in hc.locate(m2[:257, :257], "f16x3", 257))
    text = hc.describe(mask, "f16x3", K)
    assert text.startswith("3 wrong of 360000") and "tile (0, 1), wm 1, wn 0, mirrored, scalar store: 1 wrong" in text
    assert hc.describe(np.zeros((4, 4), dtype=bool), "f32", 4) == "no mismatch"


def test_the_splits_are_lossless_and_round_as_torch_does():
    r = np.random.default_rng(7)
    x = (r.standard_normal((64, 96)) * np.exp(r.uniform(-20, 20, size=(64, 96)))).astype(np.float32)
    x[0, :4] = [0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9]             # ties of the first rounding among them
    hi, mid, lo = hc.split_bf16x3(x)
    np.testing.assert_array_equal(hi + mid + lo, x.astype(np.float64))
    t = torch.from_numpy(x)
    t_hi = t.to(torch.bfloat16).float()
    t_mid = (t - t_hi).to(torch.bfloat16).float()
    t_lo = (t - t_hi - t_mid).to(torch.bfloat16).float()
    for mine, theirs in ((hi, t_hi), (mid, t_mid), (lo, t_lo)):
        assert mine.astype(np.float32).tobytes() == theirs.numpy().tobytes()
    for recipe in ("small_integers", "two_pieces", "three_pieces", "scaled(-50)", "scaled(50)", "maximum_last"):
        y = hc.RECIPES[recipe](65, 40)
        np.testing.assert_array_equal(sum(hc.split_bf16x3(y)), y.astype(np.float64))
        h, l, s = hc.split_f16x2_hessian(y, 1.0)
        np.testing.assert_array_equal(h + l, y.astype(np.float64) * s)
        ts = torch.from_numpy(y) * float(s)
        th = ts.to(torch.float16)
        tl = (ts - th.float()).to(torch.float16)
        assert h.astype(np.float16).tobytes() == th.numpy().tobytes() and l.astype(np.float16).tobytes() == tl.numpy().tobytes()
    # the scale: max |x| lands in [2^14, 2^15); the exponent is clamped at +-60 (not the piece GEMM's 110)
    assert hc.batch_scale(np.float32([[3.0]])) == 2.0 ** 13 and hc.batch_scale(np.float32([[2.0 ** 14]])) == 1.0
    assert hc.batch_scale(np.float32([[2.0 ** -100]])) == 2.0 ** 60 and hc.batch_scale(np.float32([[2.0 ** 100]])) == 2.0 ** -60
    assert hc.batch_scale(np.float32([[0.0]])) == 1.0 and hc.batch_scale(np.float32([[np.inf]])) == 1.0
    # the guard: one unit of the sample's sign where its square is alive in fp32 and hi rounded to zero; lo stays zero
    g = hc.guarded(16, 8)
    h, l, s = hc.split_f16x2_hessian(g, 1.0)
    assert s == 2.0 ** 11
    np.testing.assert_array_equal(h[:, 1], np.sign(g[:, 1]) * 2.0 ** -24)
    assert not l[:, 1].any() and not h[:, 2].any() and not h[:, 3].any() and np.signbit(h[:, 3]).all() and not np.signbit(l[:, 3]).any()
    h_off, _, _ = hc.split_f16x2_hessian(g, 0.0)
    assert not h_off[:, 1].any()
    dead = g.copy()
    dead[:, 1] = np.float32(1e-30)                                             # its square vanishes in fp32: no guard
    assert not hc.split_f16x2_hessian(dead, 1.0)[0][:, 1].any()


def test_the_host_scalars_are_powers_of_two_for_the_sample_counts_used():
    for n_seen, n_add in hc.N_TOTALS:
        n = n_seen + n_add
        assert n in (2, 8, 32) and hc.is_pow2(hc.alpha_of(n)) and hc.is_pow2(hc.sx_of(n)) and hc.sx_of(n) ** 2 == hc.alpha_of(n)
        assert hc.beta_of(n_seen, n) in (0.0, 0.5, 0.75)
    x = hc.small_integers(33, 40)
    h0 = hc.integer_h0(x, 40)
    np.testing.assert_array_equal(h0, h0.T)
    want = 0.75 * h0.astype(np.float64) + 0.25 * (x.astype(np.float64).T @ x.astype(np.float64))
    for method in hc.METHODS:
        np.testing.assert_array_equal(hc.expected(method, x, 6, 2, h0).astype(np.float64), want)


def test_the_bound_factor_is_below_the_weight_of_a_second_piece():
    """(products * padded_rows + slices + 3) 2^-24 for the tolerance shapes: at most 9 * 1024 * 2^-24 = 2^-10.8 of sum |a| |b|, a
    quarter of the 2^-8 of a hi.mid or mid.hi product.  (A lo.hi, 2^-16, is inside it: only the exact cases see that one.)"""
    for method in hc.METHODS:
        for T, K in hc.TOLERANCE_SHAPES[method]:
            rows = hc.ceil_div(T, hc.STAGE_ROWS[method]) * hc.STAGE_ROWS[method]
            assert (hc.PRODUCTS[method] * rows + 16 + 3) * 2.0 ** -24 < 2.0 ** -10


def test_the_old_h_does_not_widen_the_bound_of_the_sum():
    """With n_seen > 0 the bound is that of the sum, scaled by alpha, plus two roundings of beta h0 and nothing else."""
    x = hc.outlier_channels(512, 256)
    h0 = hc.integer_h0(x, 256)
    first, later = hc.summation_bound("f16x3", x, 0, 2, 1), hc.summation_bound("f16x3", x, 6, 2, 1, h0)
    np.testing.assert_allclose(later - 0.25 * first, 2.0 ** -23 * 0.75 * np.abs(h0), rtol=1e-6)
