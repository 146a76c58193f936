"""What the cross-compile says about csrc/qlinear_gemm.hip, without a GPU: no kernel of the file uses scratch memory or spills a
vector register, LDS stays inside 64 KiB, the products run on v_mfma_i32_16x16x64_i8, the KN staging transposes in registers
(v_perm_b32) and writes no single bytes to LDS, and the 128-row tile keeps at least two waves per SIMD."""
import re

from kernel_report import needs_hipcc, report

OCCUPANCY_128_ROW_TILE = {0: 3, 1: 4}      # waves per SIMD of ql_gemm_kernel<4, layout>: KN (130 registers), NK (124); docs/LAB_NOTES_r24.md


@needs_hipcc
def test_no_scratch_no_spills_and_the_int8_matrix_instruction():
    kernels, asm = report("qlinear_gemm.hip")
    names = {re.search(r"\d+(ql_\w+?_kernel)", n).group(1) for n in kernels}
    assert names == {"ql_gemm_kernel", "ql_reduce_kernel", "ql_sum_rows_kernel", "ql_sum_cols_kernel"}
    gemm = {name: k for name, k in kernels.items() if "ql_gemm_kernel" in name}
    assert len(gemm) == 4                                    # the 32-row and the 128-row tile x B as KN and as NK
    for name, k in kernels.items():
        assert k.scratch == 0 and k.vgpr_spill == 0 and k.sgpr_spill == 0 and k.lds <= 65536, (name, k)
    seen = {}
    for name, k in gemm.items():
        tile, layout = (int(v) for v in re.search(r"ILi(\d)ELi(\d)E", name).groups())
        assert k.occupancy >= 2 and k.vgprs <= 256, (name, k)      # __launch_bounds__(256, 2)
        assert k.lds == (32 * tile + 128) * 80, (name, k)
        if tile == 4:
            seen[layout] = k.occupancy
    assert seen == OCCUPANCY_128_ROW_TILE
    text = open(asm).read()
    assert "v_mfma_i32_16x16x64_i8" in text
    assert "v_perm_b32" in text and "ds_write_b8" not in text
    assert "v_sad_u8" in text
