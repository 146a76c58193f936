"""What the cross-compile says about csrc/matmul_nbits_fzp.hip, without a GPU: tile_gemm with the float zero point's correction
(one more MFMA per fragment of A for the row sums, a second scalar fma in the fold) still uses no scratch memory, its 128-row
kernels of a 2-byte A still fit two waves per SIMD, and neither fma of the fold is paired into v_pk_fma_f32 (docs/LAB_NOTES_r22.md:
the file is built with -fno-slp-vectorize, like its siblings)."""
import re

from kernel_report import needs_hipcc, report


@needs_hipcc
def test_no_scratch_two_waves_for_half_tiles_and_no_packed_fold():
    from onnx_quantize_amd import _build
    assert "-fno-slp-vectorize" in _build.flags_for("matmul_nbits_fzp.hip")
    kernels, asm = report("matmul_nbits_fzp.hip")
    gemm = {name: k for name, k in kernels.items() if "nbits_fzp_gemm_kernel" in name}
    assert len(gemm) == 12                                   # fp32 / fp16 / bf16 x 4 / 8 bits x the 32-row and the 128-row tile
    assert {"nbits_reduce_kernel", "nbits_split_rows_kernel"} <= {re.search(r"\d+(nbits_\w+?_kernel)", n).group(1) for n in kernels}
    for name, k in kernels.items():
        assert k.scratch == 0 and k.vgpr_spill == 0 and k.lds <= 65536, (name, k)
    for name, k in gemm.items():
        out, bits, tile = (int(v) for v in re.search(r"ILi(\d)ELi(\d)ELi(\d)E", name).groups())
        if out != 0 and tile == 4:                           # OQ_NBITS_F16 / OQ_NBITS_BF16, 128 rows
            assert k.occupancy >= 2 and k.vgprs <= 256, (name, k)
    text = open(asm).read()
    assert "v_mfma_f32_16x16x32_f16" in text and "v_mfma_f32_16x16x32_bf16" in text
    assert "v_pk_fma_f32" not in text
