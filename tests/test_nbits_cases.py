"""The helpers the MatMulNBits GPU tests stand on (tests/nbits_cases.py), checked on the host: `plan` against hand-computed plans and
against the library's workspace query, `locate` on hand-made masks, and the plan sweep's table against the properties its rows
are there for.  No kernel is launched."""
import pytest
import torch

from nbits_cases import ATYPE, DTYPES, Plan, Slot, describe, locate, plan, workspace
from test_matmul_nbits_plans_gpu import SWEEP, TWO_PIECE_SHAPES


def test_plan_on_hand_computed_shapes():
    # one 32-row tile, 4 steps, up to 8 splits wanted: one step each
    assert plan(8, 256, 16) == Plan(32, 1, 1, 4, 1, 4, 1)
    # M = 33 takes the 128-row tile; 17 steps over 8 wanted: 3 a split, 6 splits, 2 left for the last
    assert plan(33, 1088, 128) == Plan(128, 1, 1, 17, 3, 6, 2)
    # 128 tiles and more: no split, whatever K is
    assert plan(16, 4096, 16384) == Plan(32, 1, 128, 64, 64, 1, 64)
    assert plan(2048, 256, 4096) == Plan(128, 16, 32, 4, 4, 1, 4)
    # 127 tiles: 256 / 127 = 2 splits wanted
    assert plan(16, 4096, 127 * 128) == Plan(32, 1, 127, 64, 32, 2, 32)
    # K below one step
    assert plan(1, 7, 1) == Plan(32, 1, 1, 1, 1, 1, 1)
    assert plan(2048, 256, 4096).tiles == 512


def test_the_sweep_is_the_table_it_claims_to_be():
    assert [plan(*shape) for shape, _, _, _ in SWEEP] == [pl for _, _, pl, _ in SWEEP]
    assert [plan(*shape) for shape, _, _ in TWO_PIECE_SHAPES] == [pl for _, _, pl in TWO_PIECE_SHAPES]
    assert all(K <= 1344 for (_, K, _), _, _, _ in SWEEP) and 1344 * 4 * 255 * 8 < 2 ** 24            # what makes the sweep exact
    split = [(groups, pl) for _, groups, pl, _ in SWEEP if pl.splits > 1]
    assert {pl.steps_per_split for _, pl in split} == {1, 2, 3} and {pl.last for _, pl in split} == {1, 2, 3}
    # a split begins 32 mod 64 into a group, and one begins a whole number of steps into a group
    begins = {(i * pl.steps_per_split * 64) % g for groups, pl in split for g in groups for i in range(pl.splits)}
    assert any(b % 64 == 32 for b in begins) and any(b and b % 64 == 0 for b in begins)
    # one block walks several steps without slabs, on both tile heights
    assert {pl.bm for _, _, pl, _ in SWEEP if pl.splits == 1 and pl.steps > 1} == {32, 128}
    # groups that are no power of two, and a K that leaves narrow A loads
    assert {96, 160, 192} <= {g for _, groups, _, _ in SWEEP for g in groups}
    assert any(K % 8 for (_, K, _), _, _, _ in SWEEP)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_the_library_plans_what_the_helper_restates(dt):
    from onnx_quantize_amd.hip import _lib
    lib = _lib.load()
    dtype = DTYPES[dt]
    for (M, K, N), groups, pl, _ in SWEEP:
        assert lib.oq_matmul_nbits_workspace_bytes(M, K, N, groups[0], ATYPE[dtype]) == workspace(M, K, N, dtype, pl.splits)
    # the slabs are what tells one number of splits from another
    assert workspace(5, 1088, 130, torch.float16, 6) == 15616 and workspace(5, 1088, 130, torch.float16, 1) == 0
    assert workspace(5, 1088, 130, torch.float32, 6) == 2 * 11008 + 256 + 15616


def test_locate_names_the_slot_of_a_wrong_output():
    pl = plan(257, 320, 129)                                    # 128-row tiles: 3 x 2
    mask = torch.zeros(257, 129, dtype=torch.bool)
    mask[0, 0] = True
    assert locate(mask, pl) == {Slot(0, 0, 0, 0, 0, 0, 0): 1}
    mask[:] = False
    mask[256, 128] = True                                       # the one-row, one-column tail tile
    assert locate(mask, pl) == {Slot(2, 1, 0, 0, 0, 0, 0): 1}
    mask[:] = False
    # row 128 + 64 + 32 + 12: row tile 1, wave row 1, its third m-tile, row 12; columns 64 + 16 ... 31: wave column 1, second n-tile
    mask[236, 80:96] = True
    mask[238, 80:96] = True
    assert locate(mask, pl) == {Slot(1, 0, 1, 1, 2, 1, 12): 16, Slot(1, 0, 1, 1, 2, 1, 14): 16}
    text = describe(mask, pl)
    assert text.startswith("32 wrong in 2 slots") and "row [12, 14]" in text and "mt [2]" in text and "wm [1]" in text
    assert "(1, 0, 1, 1, 2, 1, 12) x16" in text
    whole = describe(torch.ones(2048, 4096, dtype=torch.bool), plan(2048, 256, 4096))          # a call that is wrong everywhere
    assert whole.startswith("8388608 wrong in 524288 slots: row_tile [0-15], col_tile [0-31], wm [0-1], wn [0-1], mt [0-3], nt [0-3], row [0-15]")
    assert describe(torch.zeros(257, 129, dtype=torch.bool), pl) == "no mismatch"


def test_locate_on_the_32_row_tile():
    pl = plan(32, 576, 260)                                     # one wave row is 16 rows: a single m-tile
    mask = torch.zeros(32, 260, dtype=torch.bool)
    mask[15, 127] = True
    mask[16, 128] = True
    mask[31, 259] = True
    assert locate(mask, pl) == {Slot(0, 0, 0, 1, 0, 3, 15): 1, Slot(0, 1, 1, 0, 0, 0, 0): 1, Slot(0, 2, 1, 0, 0, 0, 15): 1}
    # every slot of a full tile is hit exactly once per column of its 16
    counts = locate(torch.ones(32, 128, dtype=torch.bool), plan(32, 64, 128))
    assert len(counts) == 2 * 2 * 1 * 4 * 16 and set(counts.values()) == {16}
    counts = locate(torch.ones(128, 128, dtype=torch.bool), plan(128, 64, 128))
    assert len(counts) == 2 * 2 * 4 * 4 * 16 and set(counts.values()) == {16}
