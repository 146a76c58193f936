"""What the cross-compile says about csrc/matmul_nbits_decode.hip, without a GPU: the file is built unpaired (-fno-slp-vectorize)
and holds no v_pk_fma_f32, no instantiation uses scratch memory or spills a register, LDS is the slice of A and nothing else (the
blob never passes through it: fp32 on the vector ALU, 2-byte operands -- three bf16 pieces of an fp32 A -- for the matrix cores), and
the blob is read in 16-byte loads.  The register counts are in docs/LAB_NOTES_r26.md."""
import re

from kernel_report import needs_hipcc, report

SOURCE = "matmul_nbits_decode.hip"


def test_the_file_is_built_without_slp_pairing():
    from onnx_quantize_amd import _build
    assert "-fno-slp-vectorize" in _build.PER_FILE_FLAGS[SOURCE]
    assert "-fno-slp-vectorize" in _build.flags_for("/anywhere/" + SOURCE)


@needs_hipcc
def test_no_scratch_no_spills_no_paired_fma_and_the_blob_stays_out_of_lds():
    kernels, asm = report(SOURCE)
    names = {re.search(r"\d+(nbits_\w+?_kernel)", n).group(1) for n in kernels}
    assert names == {"nbits_decode_kernel", "nbits_decode_mma_kernel", "nbits_decode_reduce_kernel"}
    decode = {tuple(int(v) for v in re.search(r"ILi(\d+)ELi(\d+)ELi(\d+)E", n).groups()): k for n, k in kernels.items() if "nbits_decode_kernel" in n}
    assert sorted(decode) == [(4, 1, 4), (4, 4, 4), (4, 8, 4), (4, 16, 2), (8, 1, 4), (8, 4, 4), (8, 8, 4), (8, 16, 2)]      # (bits, row tier, rows in flight)
    for name, k in kernels.items():
        assert k.scratch == 0 and k.vgpr_spill == 0, (name, k)
        # the vector-ALU kernels spill nothing at all; the matrix-core ones park a few of their uniform values (the argument block,
        # the per-span group walk) in lanes of a vector register -- no memory is involved, ScratchSize stays 0
        assert k.sgpr_spill == 0 or ("nbits_decode_mma_kernel" in name and k.sgpr_spill <= 32), (name, k)
    for (bits, tier, rows), k in decode.items():
        assert k.lds == tier * 1024 * 4, (bits, tier, k)          # the slice of A as fp32: B is never staged
        assert k.vgprs <= 256 and k.occupancy >= 1, (bits, tier, k)
        print(f"nbits_decode_kernel<{bits}, {tier}, {rows}>: {k.vgprs} VGPRs, {k.occupancy} waves/SIMD, {k.lds} B LDS")
    mma = {tuple(int(v) for v in re.search(r"ILi(\d+)ELi(\d+)E", n).groups()): k for n, k in kernels.items() if "nbits_decode_mma_kernel" in n}
    assert sorted(mma) == [(0, 4), (0, 8), (1, 4), (1, 8), (2, 4), (2, 8)]      # (A's type code, bits)
    for (atype, bits), k in mma.items():
        assert k.lds == (3 if atype == 0 else 1) * 16 * (1024 * 2 + 16), (atype, bits, k)      # 2-byte rows padded by 16 bytes; fp32: three pieces
        assert k.vgprs <= 256 and k.occupancy >= 1, (atype, bits, k)
        print(f"nbits_decode_mma_kernel<{atype}, {bits}>: {k.vgprs} VGPRs + {k.agprs} AGPRs, {k.occupancy} waves/SIMD, {k.lds} B LDS")
    text = open(asm).read()
    assert "v_pk_fma_f32" not in text
    assert "global_load_dwordx4" in text and ("v_fma_f32" in text or "v_fmac_f32" in text)
    assert "v_mfma_f32_16x16x32_f16" in text and "v_mfma_f32_16x16x32_bf16" in text
