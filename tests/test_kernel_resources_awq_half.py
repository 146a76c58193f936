"""The kernels of csrc/awq.hip that read W, for every element type, from the compiler's own resource report (hipcc cross-compiles
without a GPU).  awq_group_diff_kernel holds a lane's 16 rows x 4 columns in registers from the load to the difference and runs
512 threads at two waves per SIMD; fp32 loads them as 16 float4, fp16 / bf16 as 16 words of 8 bytes converted at the load.  A
spilled tile keeps every parity test green at a fraction of the speed, so: no scratch, no spill, and two waves per SIMD at least,
for every instantiation.  Resource figures only; no figure of a particular compiler is written down here."""
import re

from kernel_report import needs_hipcc, report
ELEMS = ("ElemF32", "ElemF16", "ElemBF16")
TEMPLATED = ("group_absmax_kernel", "weight_scale_rows_kernel", "row_absmax_kernel", "scale_rows_kernel", "awq_diff_kernel", "awq_diff4_kernel")


@needs_hipcc
def test_awq_kernels_of_every_element_type_do_not_spill():
    seen = report("awq.hip").kernels

    # the fused quantize-residual kernel: <element, PIECES> for three elements and both values of PIECES
    fused = {k: v for k, v in seen.items() if "awq_group_diff_kernel" in k}
    built = sorted((e, p) for k in fused for e in ELEMS for p in (0, 1) if re.search(r"awq_group_diff_kernelINS_\d+%sELb%dE" % (e, p), k))
    assert built == sorted((e, p) for e in ELEMS for p in (0, 1)), sorted(fused)
    assert len(fused) == 6, sorted(fused)
    for name, k in fused.items():
        assert k.scratch == 0 and k.sgpr_spill == 0 and k.vgpr_spill == 0, (name, k)
        assert k.occupancy >= 2, (name, k)

    # every other kernel that reads W: fp32, fp16, bf16, none of them with scratch
    for key in TEMPLATED:
        mine = {k: v for k, v in seen.items() if re.search(r"\d+%sINS_" % key, k)}
        assert sorted(e for k in mine for e in ELEMS if re.search(r"%sINS_\d+%sEE" % (key, e), k)) == sorted(ELEMS), (key, sorted(mine))
        for name, k in mine.items():
            assert k.scratch == 0 and k.sgpr_spill == 0 and k.vgpr_spill == 0, (name, k)
