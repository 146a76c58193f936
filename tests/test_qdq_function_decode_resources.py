"""What the cross-compile says about csrc/qdq_function_decode.hip, without a GPU: no kernel of the file uses scratch memory or spills
a vector register, the four product kernels keep two waves per SIMD next to their 64 load registers, and the product is
v_mfma_i32_16x16x64_i8.  The register counts are in docs/LAB_NOTES_r47.md."""
import re

from kernel_report import needs_hipcc, report

SOURCE = "qdq_function_decode.hip"
KERNELS = {"qq_minmax_rows_kernel", "qq_params_kernel", "qq_quantize_rows_kernel", "qfd_product_kernel", "qq_reduce_kernel", "qq_finish_dynamic_kernel"}


@needs_hipcc
def test_no_scratch_no_vector_spills_and_two_waves_per_simd():
    kernels, asm = report(SOURCE)
    short = lambda name: re.search(r"\d+(q\w+?_kernel)", name).group(1)      # noqa: E731
    assert {short(n) for n in kernels} == KERNELS
    for name, k in sorted(kernels.items()):
        print(f"{short(name)}{tuple(re.findall('Lb([01])E', name))}: {k.vgprs} VGPRs + {k.agprs} AGPRs, {k.occupancy} waves/SIMD, {k.lds} B LDS")
        assert k.scratch == 0 and k.vgpr_spill == 0 and k.lds <= 64 * 1024, (name, k)
    product = [k for n, k in kernels.items() if short(n) == "qfd_product_kernel"]
    assert len(product) == 4 and all(k.occupancy >= 2 for k in product)      # with / without the row sums x with / without the column sums
    assert "v_mfma_i32_16x16x64_i8" in open(asm).read()
