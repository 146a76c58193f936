"""The kernels of csrc/rtn_mse.hip for every element type, from the compiler's own resource report (hipcc cross-compiles
without a GPU).  mse_rows_reg_kernel holds a group's values in registers across the 20 candidates: fp32 as they are, fp16 / bf16
converted at the load for groups of up to 128, and PACKED two per register for groups of 256 (which exist for the 2-byte types
only).  A spilled tile keeps every parity test green at a fraction of the speed, so: no scratch, no spill, and two waves per
SIMD at least.  Resource figures only; no figure of a particular compiler is written down here."""
import re

from kernel_report import ALL_ELEMS, element_types, needs_hipcc, report
FP32_GROUPS = (32, 64, 128)
HALF_GROUPS = (32, 64, 128, 256)


@needs_hipcc
def test_mse_register_tiles_of_every_element_type_do_not_spill():
    seen = report("rtn_mse.hip").kernels
    tiles = {k: v for k, v in seen.items() if "mse_rows_reg_kernel" in k}

    def built(elem):
        """Group sizes instantiated for an element type, from the mangled template arguments <oq::Elem, G>."""
        return sorted(int(m.group(1)) for m in (re.search(r"mse_rows_reg_kernelINS_\d+%sELi(\d+)E" % elem, k) for k in tiles) if m)

    assert built("ElemF32") == list(FP32_GROUPS), sorted(tiles)                     # still three: no fp32 tile of 256
    assert built("ElemF16") == built("ElemBF16") == list(HALF_GROUPS), sorted(tiles)
    assert len(tiles) == len(FP32_GROUPS) + 2 * len(HALF_GROUPS), sorted(tiles)
    for name, k in tiles.items():
        assert k.scratch == 0 and k.sgpr_spill == 0 and k.vgpr_spill == 0, (name, k)
        assert k.occupancy >= 2, (name, k)
    for key in ("mse_rows_kernel", "mse_tensor_partial", "tensor_minmax_kernel"):  # fp32, fp16, bf16
        assert element_types(seen, key) == ALL_ELEMS, (key, sorted(seen))
    for key in ("mse_tensor_mask", "mse_resolve_kernel"):                          # they never see W
        assert sum(key in k for k in seen) == 1, (key, sorted(seen))
