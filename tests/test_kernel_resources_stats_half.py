"""The kernels of csrc/abs_stats_half.hip (oq_abs_stats_cols_many_h16) from the compiler's own resource report (hipcc
cross-compiles without a GPU): HBM-bound streams that keep 8 or 16 row loads in flight per lane, so scratch traffic would compete
with the stream itself.  No figure of a particular compiler is written down here: no scratch, no spill, and a 256-thread block
must fit a SIMD's share of the registers at all."""
from kernel_report import HALF_ELEMS, element_types, needs_hipcc, report


@needs_hipcc
def test_abs_stats_kernels_have_no_scratch():
    seen, asm_path = report("abs_stats_half.hip")
    assert element_types(seen, "abs_stats_half_partial") == HALF_ELEMS, list(seen)
    assert sum("abs_stats_half_fold" in name for name in seen) == 1, list(seen)
    assert len(seen) == 3, list(seen)
    for name, k in seen.items():
        assert k.scratch == 0 and k.sgpr_spill == 0 and k.vgpr_spill == 0, (name, k)
        assert k.occupancy >= 1, (name, k)
    with open(asm_path) as f:
        asm = f.read()
    assert "flat_load" not in asm and "flat_store" not in asm              # table pointers are used as global memory
