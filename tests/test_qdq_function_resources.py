"""What the cross-compile says about csrc/qdq_function.hip, without a GPU: no kernel of the file uses scratch memory or spills a
vector register, LDS stays within 64 KiB, the tile kernels keep two waves per SIMD and the LDS of their twins in
csrc/qlinear_function.hip, and the product is v_mfma_i32_16x16x64_i8.  The register counts are in docs/LAB_NOTES_r36.md."""
import re

from kernel_report import needs_hipcc, report

SOURCE = "qdq_function.hip"
KERNELS = {"qq_minmax_rows_kernel", "qq_params_kernel", "qq_quantize_rows_kernel", "qq_sum_cols_kernel", "qq_gemm_kernel", "qq_reduce_kernel",
           "qq_finish_dynamic_kernel"}


def test_the_file_is_built_like_the_rest_of_the_library():
    from onnx_quantize_amd import _build
    flags = _build.flags_for("/anywhere/" + SOURCE)
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags
    assert flags == _build.flags_for("/anywhere/qlinear_gemm.hip") == _build.flags_for("/anywhere/qlinear_function.hip")
    assert SOURCE not in _build.PER_FILE_FLAGS


def short(name):
    return re.search(r"\d+(qq_\w+?_kernel)", name).group(1)


@needs_hipcc
def test_no_scratch_no_vector_spills_lds_and_occupancy():
    kernels, asm = report(SOURCE)
    assert {short(n) for n in kernels} == KERNELS
    for name, k in sorted(kernels.items()):
        args = tuple(int(v) for v in re.findall(r"L[ib](\d+)E", name))
        print(f"{short(name)}{args}: {k.vgprs} VGPRs + {k.agprs} AGPRs, {k.occupancy} waves/SIMD, "
              f"{k.lds} B LDS, {k.sgpr_spill} SGPR spills")
        assert k.scratch == 0 and k.vgpr_spill == 0, (name, k)
        assert k.lds <= 64 * 1024, (name, k)
        assert k.vgprs <= 256 and k.occupancy >= 1, (name, k)
    gemm = sorted((k.lds, k) for n, k in kernels.items() if short(n) == "qq_gemm_kernel")
    assert len(gemm) == 2                                                                  # the 32- and the 128-row tile, B in KN
    theirs, _ = report("qlinear_function.hip")
    twins = sorted({k.lds for n, k in theirs.items() if "qf_gemm_kernel" in n})
    assert [lds for lds, _ in gemm] == twins                                               # the epilogue's fold reuses the tiles' LDS
    for _, k in gemm:
        assert k.occupancy >= 2, k
    assert "v_mfma_i32_16x16x64_i8" in open(asm).read()
