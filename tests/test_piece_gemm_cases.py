"""The vocabulary of the fp16-piece GEMM tests (piece_gemm_cases.py) checked on the CPU: every exact case the GPU file uses satisfies
`exact_ok` and is reproduced by `emulate` to the bit, the condition bites, `locate` names the slot of hand-placed errors, and
`emulate` alone stays inside the representation bound its module docstring derives on every random case the GPU file uses."""
import numpy as np
import pytest

import piece_gemm_cases as pg


@pytest.mark.parametrize("case", pg.exact_cases(), ids=[f"{name}-{'x'.join(map(str, shape))}-{'row' if per_row else 'operand'}"
                                                        for name, shape, per_row in pg.exact_cases()])
def test_every_exact_case_of_the_gpu_file_is_exact(case):
    name, shape, per_row = case
    a, b = pg.RECIPES[name](*shape)
    assert a.shape == shape[:2] and b.shape == shape[1:] and a.dtype == b.dtype == np.float32
    assert pg.exact_ok(a, b, per_row)
    em = pg.emulate(a, b, per_row)
    want = a.astype(np.float64) @ b.astype(np.float64)
    assert np.array_equal(em.y, want) and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    a2, b2 = pg.RECIPES[name](*shape)
    assert np.array_equal(a, a2) and np.array_equal(b, b2)            # seeded by (recipe, shape)


def test_the_recipes_hold_what_they_say():
    a, b = pg.a_two_pieces(70, 1000, 37)
    _, la, _ = pg.split(a, True)
    _, lb, _ = pg.split(b.T, False)
    assert np.abs(a).max() > 4096 and 0.15 < (la != 0).mean() < 0.35 and not lb.any()          # about a quarter of A has a lo
    a, b = pg.b_two_pieces(70, 1000, 37)
    assert not pg.split(a, True)[1].any() and 0.15 < (pg.split(b.T, False)[1] != 0).mean() < 0.35
    a, b = pg.one_piece(70, 1000, 37)
    assert not pg.split(a, True)[1].any() and not pg.split(b.T, False)[1].any()
    a, b = pg.both_two_pieces(70, 1000, 37)
    la, lb = pg.split(a, True)[1], pg.split(b.T, False)[1].T
    assert la[:, 0::2].any() and not la[:, 1::2].any() and lb[1::2].any() and not lb[0::2].any()
    assert (la @ np.abs(pg.split(b.T, False)[0].T)).any() and (np.abs(pg.split(a, True)[0]) @ lb).any()      # both cross products live
    a, b = pg.full_width(70, 1000, 37)
    ha, la, s = pg.split(a, False)
    assert s.item() == 2.0 ** -6 and np.all(a % 2 != 0) and np.abs(a).max() == 2 ** 21 - 1
    assert np.abs(ha).max() == 2.0 ** 15 and np.abs(la).max() >= 7.5 and pg.lowest_set_bit(ha, la).min() == 2.0 ** -6     # all 22 bits
    assert np.array_equal((b != 0).sum(axis=0), np.full(37, 7)) and set(np.unique(b)) == {-1.0, 0.0, 1.0}
    for shape in ((70, 1000, 37), (2081, 2081, 8)):
        em = pg.emulate(*pg.one_piece(*shape), True)
        assert 2.0 ** 20 < em.units.max() < 2.0 ** 24, em.units.max()


def test_the_condition_bites():
    """`full_width` with an eighth nonzero per column: 8 (2^21 + 1) units in row 0, and `exact_ok` says no; so it does for a
    lo . lo product that does not vanish, and for an element of more than 22 bits."""
    a, b = pg.full_width(70, 1000, 37, per_column=8)
    em = pg.emulate(a, b, True)
    assert em.lossless and not em.lolo.any() and em.units[0].min() == 8 * (2.0 ** 21 + 1)
    assert not pg.exact_ok(a, b, True) and not pg.exact_ok(a, b, False)
    assert pg.exact_ok(*pg.full_width(70, 1000, 37), False)
    a, b = pg.a_two_pieces(70, 100, 37)
    assert pg.exact_ok(a, b, True)
    b[3, 5] = 4099.0                                                    # B needs a lo as well: lo_a lo_b is dropped
    em = pg.emulate(a, b, True)
    assert em.lossless and em.lolo[:, 5].any() and not pg.exact_ok(a, b, True)
    a, b = pg.one_piece(70, 100, 37)
    a[0, 0] = float(0xAAAAAB)                                           # 24 bits: lo would need twelve
    assert not pg.emulate(a, b, True).lossless and not pg.exact_ok(a, b, True)


def test_the_split_restates_the_scale_rules():
    x = np.array([[3.0, -5.0, 0.0], [0.0, 0.0, 0.0], [np.inf, 1.0, 2.0], [np.nan, 1.0, 2.0], [1e-38, 0.0, 0.0], [3e38, 1.0, 0.0]], dtype=np.float32)
    hi, lo, s = pg.split(x, True)
    assert s[:, 0].tolist() == [2.0 ** 12, 1.0, 1.0, 1.0, 2.0 ** 110, 2.0 ** -110]          # 5 = 0.625 * 2^3; zero, Inf, NaN: 1; both clamps
    assert np.array_equal(hi[0], [3 * 4096.0, -5 * 4096.0, 0.0]) and not lo[:2].any()
    assert np.isinf(hi[2, 0]) and np.isnan(lo[2, 0]) and np.isnan(hi[3, 0])
    assert pg.scale_is_clamped(x[4:5], True).all() and pg.scale_is_clamped(x[5:6], True).all() and not pg.scale_is_clamped(x[:1], True).any()
    _, _, s = pg.split(x[:2], False)
    assert s.shape == (1, 1) and s.item() == 2.0 ** 12
    assert pg.split(x, False)[2].item() == 1.0                         # a non-finite maximum: the operand's scale falls to 1
    hi, lo, s = pg.split(np.array([[4099.0, 1.0]], dtype=np.float32), True)                    # 4099 * 4 = 16396 = 16400 - 4: round to even
    assert s.item() == 4.0 and hi[0].tolist() == [16400.0, 4.0] and lo[0].tolist() == [-4.0, 0.0]


def test_the_cases_beyond_2048_rows_are_exact_and_a_missed_maximum_overflows():
    for which in "ab":
        a, b, per_row = pg.beyond_2048_rows(which)
        assert pg.exact_ok(a, b, per_row)
        src = b if which == "b" else a
        assert src.shape[0] == 2081 and np.abs(src[:2080]).max() < np.abs(src[2080]).max()
        s_missed = pg.pow2_scale(np.abs(src[:2048]).max())
        assert np.abs(src).max() * s_missed >= 65520.0                  # rounds to infinity in fp16


def test_the_parts_of_the_split_contraction_are_exact():
    a, b = pg.a_two_pieces(*pg.FORMS_SHAPE)
    assert pg.exact_ok(a[:, :40], b[:40], True) and pg.exact_ok(a[:, 40:], b[40:], True)


def test_the_epilogue_condition():
    for N in (36, 37):
        a, b = pg.a_two_pieces(70, 100, N)
        c = pg.integer_c(70, N)
        assert np.abs(c).max() == 2000 and np.all(c % 2 == 0)
        for alpha in (1.0, -1.0, 0.25, 3.0):
            for beta in (1.0, 0.5, -2.0):
                assert pg.epilogue_ok(a, b, True, alpha, beta, c)
    assert not pg.epilogue_ok(a, b, True, 99.0, 1.0, c)                # 99 sum |a| |b| > 2^24
    assert not pg.epilogue_ok(a, b, True, 1.0, 2.0 ** -12, c)          # the unit falls to 2^-11


# ------------------------------------------------------------------------------------ locate
def test_locate_names_the_slot_of_hand_placed_errors():
    M, N = 257, 513
    V, S = "vector", "scalar"
    placed = {(0, 0): pg.Slot(0, 0, 0, 0, 0, 0, 0, 0, S, False), (0, 512): pg.Slot(0, 2, 0, 0, 0, 0, 0, 0, S, True),
              (256, 0): pg.Slot(1, 0, 0, 0, 0, 0, 0, 0, S, False), (256, 512): pg.Slot(1, 2, 0, 0, 0, 0, 0, 0, S, True),
              (255, 511): pg.Slot(0, 1, 3, 1, 3, 7, 3, 15, S, False), (100, 300): pg.Slot(0, 1, 1, 0, 2, 2, 1, 12, S, False),
              (77, 130): pg.Slot(0, 0, 1, 1, 0, 0, 3, 2, S, False)}
    for (r, c), slot in placed.items():
        mask = np.zeros((M, N), dtype=bool)
        mask[r, c] = True
        assert pg.locate(mask) == {slot: 1}, (r, c)                    # ldc = 513: no vector stores at all
        vec = slot._replace(store=S if slot.last_group else V)
        assert pg.locate(mask, ldc=516) == {vec: 1}, (r, c)            # ldc % 4 == 0: vectors but in the last, partial group
        assert pg.locate(mask, ldc=516, aligned=False) == {slot: 1}
    mask = np.zeros((M, N), dtype=bool)
    for r, c in placed:
        mask[r, c] = True
    assert pg.locate(mask) == {slot: 1 for slot in placed.values()}
    # a whole wave's quarter of MFMA tile column j = 7: twelve wrong in one (kc, cl) each
    mask = np.zeros((300, N), dtype=bool)
    mask[256 + 0:256 + 4, 256 + 128 + 7 * 16 + 4:256 + 128 + 7 * 16 + 7] = True
    got = pg.locate(mask, ldc=516)
    assert got == {pg.Slot(1, 1, 0, 1, 0, 7, 0, cl, V, False): 4 for cl in (4, 5, 6)}
    text = pg.describe(mask, ldc=516)
    assert "tile (1, 1), wm 0, wn 1, j 7, vector store: 12 wrong" in text and text.startswith("12 wrong in 1 groups"), text
    assert "scalar store: 12 wrong" in pg.describe(mask, ldc=517)
    assert pg.describe(np.zeros((3, 3), dtype=bool)) == "no mismatch" and pg.locate(np.zeros((3, 3), dtype=bool)) == {}
    # N % 4 == 0: no partial group; a swapped tile_m / tile_n shows in the tile coordinates
    mask = np.zeros((512, 768), dtype=bool)
    mask[:256, 256:512] = True
    assert {(s.tile_m, s.tile_n) for s in pg.locate(mask)} == {(0, 1)} and not any(s.last_group for s in pg.locate(mask))
    assert pg.compact([0, 1, 2, 3, 7]) == "[0-3, 7]"


# ------------------------------------------------------------------------------------ the representation bound
def test_the_element_bound_is_the_stated_one_while_the_scale_is_not_clamped():
    r = np.random.default_rng(5)
    x = (r.standard_normal((64, 512)) * np.exp(r.uniform(-10, 10, size=(64, 1)))).astype(np.float32)
    x[:, 7] *= 2.0 ** -20                                                # elements far below their row: the subnormal term
    for per_row in (True, False):
        hi, lo, s = pg.split(x, per_row)
        m = np.abs(x).max(axis=1, keepdims=True) if per_row else np.abs(x).max()
        err = np.abs(x.astype(np.float64) - (hi + lo) / s)
        stated = 2.0 ** -22 * np.abs(x.astype(np.float64)) + 2.0 ** -39 * m
        assert not pg.scale_is_clamped(x, per_row).any()
        assert np.all(pg.element_bound(x, per_row) <= stated) and np.all(err <= pg.element_bound(x, per_row))
        assert (err > 2.0 ** -22 * np.abs(x)).any()                     # the second term is needed


@pytest.mark.parametrize("case", pg.magnitude_cases(), ids=[f"{kind}-{'x'.join(map(str, shape))}-{'row' if per_row else 'operand'}"
                                                            for kind, shape, per_row in pg.magnitude_cases()])
def test_emulate_stays_inside_the_representation_bound(case):
    kind, shape, per_row = case
    a, b = pg.magnitude_case(kind, shape)
    em = pg.emulate(a, b, per_row)
    want = a.astype(np.float64) @ b.astype(np.float64)
    bound = pg.representation_bound(a, b, per_row)
    err = np.abs(em.y - want)
    print(f"{kind} {shape} per_row={per_row}: max err / bound = {(err / bound).max():.3f}, "
          f"max err / (2^-22 sum|a||b|) = {(err / (np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64)))).max() * 2.0 ** 22:.3f}")
    assert np.isfinite(em.y).all() and np.all(err <= bound)
    clamped = pg.scale_is_clamped(a, per_row).any() or pg.scale_is_clamped(b.T, False).any()
    assert clamped == (kind in ("a 1e-30", "b 1e-30")), "only the 1e-30 operands reach the clamp of the scale"
    live = em.mass > 0                                                 # (an operand-scale row 10^18 below the largest vanishes whole)
    assert np.all((pg.summation_bound(em, shape[1]) < 2.0 ** -11 * em.mass / (em.s_a * em.s_b))[live])      # a dropped piece would show


def test_the_sample_of_the_issue():
    """64 x 512 x 40 with a row spread of e^+-10: the error of `emulate` is a small fraction of 2^-22 sum |a| |b|."""
    r = np.random.default_rng(1)
    a = (r.standard_normal((64, 512)) * np.exp(r.uniform(-10, 10, size=(64, 1)))).astype(np.float32)
    b = (r.standard_normal((512, 40)) / 32).astype(np.float32)
    em = pg.emulate(a, b, True)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    err = np.abs(em.y - a64 @ b64)
    assert np.all(err <= pg.representation_bound(a, b, True)) and (err / (np.abs(a64) @ np.abs(b64))).max() < 0.5 * 2.0 ** -22


def test_the_buffer_formula():
    assert pg.pieces_bytes_at_least(1, 1) == 4 * 2 * 256 * 16 + 16384 + 8
    assert pg.pieces_bytes_at_least(33, 257) == 2 * 4 * 2 * 512 * 16 + 16384 + 8 * 257
