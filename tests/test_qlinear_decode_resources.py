"""What the cross-compile says about csrc/qlinear_decode.hip, without a GPU: no instantiation uses scratch memory or spills a
register, LDS stays within 64 KiB (A's slice, and for a KN matrix the hand-over of three waves' sums in the same buffer: B never
passes through it), the products are signed dot4 instructions and -- the 8- and 16-row tiers of an NK matrix -- v_mfma_i32_16x16x64_i8,
a KN matrix is transposed with v_perm_b32, and an NK one is read in 16-byte loads.  The register counts are in docs/LAB_NOTES_r27.md."""
import re

from kernel_report import needs_hipcc, report

SOURCE = "qlinear_decode.hip"
TIERS = [1, 4, 8, 16]


def test_the_file_is_built_like_the_rest_of_the_library():
    from onnx_quantize_amd import _build
    flags = _build.flags_for("/anywhere/" + SOURCE)
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags


@needs_hipcc
def test_no_scratch_no_spills_lds_within_64k_and_the_chosen_instructions():
    kernels, asm = report(SOURCE)
    names = {re.search(r"\d+(ql_decode_\w+?_kernel)", n).group(1) for n in kernels}
    assert names == {"ql_decode_nk_kernel", "ql_decode_nk_mma_kernel", "ql_decode_kn_kernel", "ql_decode_reduce_kernel"}
    for name, k in kernels.items():
        # nothing goes to memory.  The NK kernels park a few uniform values (the argument block next to the guarded loads' state; on the
        # matrix cores the 16 spans' guards) in lanes of a vector register: no memory is involved, ScratchSize stays 0
        assert k.scratch == 0 and k.vgpr_spill == 0 and k.sgpr_spill <= (64 if "nk_mma" in name else 8), (name, k)
        assert k.lds <= 64 * 1024, (name, k)
        assert k.vgprs <= 256 and k.occupancy >= 1, (name, k)
    for route in ("nk", "kn"):
        found = {}
        for n, k in kernels.items():
            if f"ql_decode_{route}_kernel" in n:
                tier, cs = re.search(r"ILi(\d+)ELb([01])E", n).groups()
                found[(int(tier), int(cs))] = k
        assert sorted(found) == [(t, cs) for t in TIERS for cs in (0, 1)]                # (row tier, column sums taken)
        for (tier, cs), k in sorted(found.items()):
            # the slice of A as bytes (KN: or, in the same buffer, three waves' sums on their way to wave 0) and up to 16 row sums:
            # B is never staged
            buffer = tier * 1024 if route == "nk" else max(tier * 1024, 3 * 64 * (tier * 4 + 4 * cs) * 4)
            assert buffer < k.lds <= buffer + 16 * 4, (route, tier, cs, k)
            print(f"ql_decode_{route}_kernel<{tier}, {bool(cs)}>: {k.vgprs} VGPRs + {k.agprs} AGPRs, {k.occupancy} waves/SIMD, {k.lds} B LDS")
    mma = {int(re.search(r"ILb([01])E", n).group(1)): k for n, k in kernels.items() if "ql_decode_nk_mma_kernel" in n}
    assert sorted(mma) == [0, 1]
    for cs, k in sorted(mma.items()):
        assert 16 * (1024 + 16) < k.lds <= 16 * (1024 + 16) + 16 * 4, (cs, k)         # 16 rows of A padded by 16 bytes, and their sums
        print(f"ql_decode_nk_mma_kernel<{bool(cs)}>: {k.vgprs} VGPRs + {k.agprs} AGPRs, {k.occupancy} waves/SIMD, {k.lds} B LDS")
    text = open(asm).read()
    assert re.search(r"\bv_dot4c?_i32_i8", text), "the products are signed dot4 instructions"
    assert "v_perm_b32" in text and "global_load_dwordx4" in text
    assert "v_mfma_i32_16x16x64_i8" in text                                               # the decision of docs/LAB_NOTES_r27.md
