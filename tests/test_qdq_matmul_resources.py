"""What the cross-compile says about csrc/qdq_matmul.hip, without a GPU: no kernel of the file uses scratch memory or spills a
vector register, the 128-row kernels of a 2-byte A fit two waves per SIMD, and the per-group fold is NOT paired into
v_pk_fma_f32 -- the paired fold gave wrong sums on the MI355X (docs/LAB_NOTES_r22.md), which is why the file is built with
-fno-slp-vectorize from its first compile.  The same of csrc/matmul_nbits.hip, whose kernels are tile_gemm
(csrc/nbits_tile.hpp), the body this file's kernel has a copy of.  `python tests/test_qdq_matmul_resources.py` prints the figures the README
rows record."""
import re

from kernel_report import needs_hipcc, report


def gemm_kernels():
    kernels, asm = report("qdq_matmul.hip")
    return {name: k for name, k in kernels.items() if "qdq_gemm_kernel" in name}, kernels, asm


@needs_hipcc
def test_no_scratch_no_spills_two_waves_for_half_tiles_and_no_packed_fold():
    from onnx_quantize_amd import _build
    assert "-fno-slp-vectorize" in _build.flags_for("qdq_matmul.hip")
    gemm, kernels, asm = gemm_kernels()
    assert len(gemm) == 6                                    # fp32 / fp16 / bf16 x the 32-row and the 128-row tile
    # the reduce and split-rows kernels are those of matmul_nbits.hip, instantiated from the shared header
    assert {"nbits_reduce_kernel", "nbits_split_rows_kernel"} <= {m.group(1) for m in (re.search(r"\d+(nbits_\w+?_kernel)", n) for n in kernels) if m}
    for name, k in kernels.items():
        assert k.scratch == 0 and k.vgpr_spill == 0 and k.lds <= 65536, (name, k)
    for name, k in gemm.items():
        out, tile = (int(v) for v in re.search(r"ILi(\d)ELi(\d)E", name).groups())
        if out != 0 and tile == 4:                           # OQ_NBITS_F16 / OQ_NBITS_BF16, 128 rows
            assert k.occupancy >= 2 and k.vgprs <= 256, (name, k)
    text = open(asm).read()
    assert "v_mfma_f32_16x16x32_f16" in text and "v_mfma_f32_16x16x32_bf16" in text and "v_perm_b32" in text
    assert "v_pk_fma_f32" not in text


@needs_hipcc
def test_the_blob_kernels_keep_the_same_bounds():
    from onnx_quantize_amd import _build
    assert "-fno-slp-vectorize" in _build.flags_for("matmul_nbits.hip")
    kernels, asm = report("matmul_nbits.hip")
    gemm = {name: k for name, k in kernels.items() if "nbits_gemm_kernel" in name}
    assert len(gemm) == 12                                   # fp32 / fp16 / bf16 x 4 / 8 bits x the 32-row and the 128-row tile
    for name, k in gemm.items():
        out, bits, tile = (int(v) for v in re.search(r"ILi(\d)ELi(\d)ELi(\d)E", name).groups())
        assert k.lds <= 65536, (name, k)
        if out != 0:                                         # OQ_NBITS_F16 / OQ_NBITS_BF16: a 2-byte A
            assert k.scratch == 0 and k.vgpr_spill == 0, (name, k)
            assert k.occupancy >= 2 and k.vgprs <= 256, (name, k)
    text = open(asm).read()
    assert "v_mfma_f32_16x16x32_f16" in text and "v_mfma_f32_16x16x32_bf16" in text
    assert "v_pk_fma_f32" not in text


if __name__ == "__main__":
    for name, k in sorted(gemm_kernels()[0].items()):
        print(re.search(r"ILi(\d)ELi(\d)E", name).groups(), k)
    for name, k in sorted(report("matmul_nbits.hip").kernels.items()):
        if "nbits_gemm_kernel" in name:
            print(re.search(r"ILi(\d)ELi(\d)ELi(\d)E", name).groups(), k)
