"""`rtn_group_wave_pair` (csrc/rtn.hip), the headline launch since round 44, sits at the same register boundary as the four-wave
build it shares its body with: <= 96 VGPRs for five waves per SIMD, no scratch.  Its LDS -- 16 KB of lines, 1 KB of scales, 256 B of
zero points -- has to stay far from what would bound the two eight-wave blocks a CU holds."""
from kernel_report import needs_hipcc, report


@needs_hipcc
def test_pair_kernel_keeps_the_registers_of_five_waves_per_simd():
    k = report("rtn.hip").kernels["_ZN2oq19rtn_group_wave_pairENS_7RtnArgsE"]
    assert k.vgprs <= 96 and k.occupancy >= 5 and k.vgpr_spill == 0 and k.scratch == 0, k
    assert k.lds <= 16384 + 1024 + 256, k
