"""What the cross-compile says about csrc/qlinear_function.hip, without a GPU: no kernel of the file uses scratch memory or spills a
vector register, LDS stays within 64 KiB, the decode kernels keep the LDS of their byte-staging twins in csrc/qlinear_decode.hip
(A's slice is still bytes: the quantizer sits in front of LDS), the tile kernels keep two waves per SIMD, and the products are
v_mfma_i32_16x16x64_i8 and signed dot4 instructions.  The register counts are in docs/LAB_NOTES_r32.md."""
import re

from kernel_report import needs_hipcc, report

SOURCE = "qlinear_function.hip"
TIERS = [1, 4, 8, 16]


def test_the_file_is_built_like_the_rest_of_the_library():
    from onnx_quantize_amd import _build
    flags = _build.flags_for("/anywhere/" + SOURCE)
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags
    assert flags == _build.flags_for("/anywhere/qlinear_gemm.hip") == _build.flags_for("/anywhere/qlinear_decode.hip")
    assert SOURCE not in _build.PER_FILE_FLAGS


def short(name):
    return re.search(r"\d+(qf_\w+?_kernel)", name).group(1)


def template_args(name):
    """The integer / bool template arguments of a mangled kernel name, in order."""
    return tuple(int(v) for v in re.findall(r"L[ib](\d+)E", name))


@needs_hipcc
def test_no_scratch_no_vector_spills_lds_and_occupancy():
    kernels, asm = report(SOURCE)
    assert {short(n) for n in kernels} == {"qf_quantize_rows_kernel", "qf_gemm_kernel", "qf_reduce_kernel", "qf_sum_rows_kernel", "qf_sum_cols_kernel",
                                           "qf_decode_nk_kernel", "qf_decode_nk_mma_kernel", "qf_decode_kn_kernel", "qf_decode_reduce_kernel"}
    for name, k in sorted(kernels.items()):
        print(f"{short(name)}{template_args(name)}: {k.vgprs} VGPRs + {k.agprs} AGPRs, {k.occupancy} waves/SIMD, {k.lds} B LDS, "
              f"{k.sgpr_spill} SGPR spills")
        assert k.scratch == 0 and k.vgpr_spill == 0, (name, k)
        assert k.lds <= 64 * 1024, (name, k)
        assert k.vgprs <= 256 and k.occupancy >= 1, (name, k)
    gemm = [k for n, k in kernels.items() if short(n) == "qf_gemm_kernel"]
    assert len(gemm) == 4                                                                  # 32- and 128-row tiles x both layouts of B
    for k in gemm:
        assert k.occupancy >= 2, k
    text = open(asm).read()
    assert "v_mfma_i32_16x16x64_i8" in text
    assert re.search(r"\bv_dot4c?_i32_i8", text), "the decode products are signed dot4 instructions"


@needs_hipcc
def test_the_decode_kernels_keep_the_lds_of_their_byte_staging_twins():
    ours, _ = report(SOURCE)
    theirs, _ = report("qlinear_decode.hip")
    twins = {"qf_decode_nk_kernel": "ql_decode_nk_kernel", "qf_decode_nk_mma_kernel": "ql_decode_nk_mma_kernel", "qf_decode_kn_kernel": "ql_decode_kn_kernel"}
    byte_route = {(re.search(r"\d+(ql_decode_\w+?_kernel)", n).group(1), template_args(n)): k for n, k in theirs.items()}
    seen = 0
    for name, k in ours.items():
        if short(name) in twins:
            twin = byte_route[(twins[short(name)], template_args(name))]
            assert k.lds == twin.lds, (name, k, twin)
            seen += 1
    assert seen == 2 * len(TIERS) * 2 + 2                                                  # NK and KN x four tiers x column sums, and the two MFMA kernels
