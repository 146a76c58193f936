"""Occupancy guard for the two headline RTN kernels.  Both sit right at a register boundary of the gfx950 allocation table
(MI355X_MICROARCH.md, Register files): `rtn_group_wave<8, true, 5>` needs <= 96 VGPRs for five waves per SIMD (92 today; the
plain build has 100), `rtn_group_fused<16, ...>` needs <= 128 for four (126 today).  Four registers more in the fused
kernel cost 30 % of its time in round 2 (44.6 -> 58.5 us) without a single test failing, so the compiler's own resource
report is checked here (hipcc cross-compiles without a GPU)."""
import re

import pytest

from kernel_report import needs_hipcc, report


@needs_hipcc
def test_headline_kernels_keep_their_occupancy():
    seen = report("rtn.hip").kernels
    wave = seen["_ZN2oq14rtn_group_waveILi8ELb1ELi5EEEvNS_7RtnArgsE"]            # MatMulNBits blob, g = 128: the headline launch
    fused = seen["_ZN2oq15rtn_group_fusedILi16ELb1ELb1ELb0EEEvNS_7RtnArgsE"]     # [K, N] bytes, g = 128
    fused_tr = seen["_ZN2oq15rtn_group_fusedILi16ELb1ELb1ELb1EEEvNS_7RtnArgsE"]  # the same with the parameters transposed inside the launch
    assert fused_tr.vgprs <= 128 and fused_tr.occupancy >= 4 and fused_tr.vgpr_spill == 0, fused_tr
    assert wave.vgprs <= 96 and wave.occupancy >= 5 and wave.vgpr_spill == 0, wave
    assert fused.vgprs <= 128 and fused.occupancy >= 4 and fused.vgpr_spill == 0, fused
    for name, k in seen.items():
        assert k.vgpr_spill == 0, (name, k)                                            # no kernel of the file may spill


@needs_hipcc
def test_hessian_gemm_kernels_fit_two_waves_per_simd_without_spilling():
    """The split-operand SYRK kernels run one 8-wave block per CU (two waves per SIMD: <= 256 registers) with all 128
    accumulator registers live across the stage loop: a spill there would sit inside the MFMA stream."""
    seen = 0
    for name, k in report("syrk_bf16x3.hip").kernels.items():
        if any(key in name for key in ("syrk_pieces_kernel", "syrk_f16_m16_kernel", "syrk_f16_m16_many_kernel", "gemm_f16x3_kernel", "gemm_f16x3_many_kernel")):
            seen += 1
            assert k.vgprs <= 256 and k.scratch == 0 and k.occupancy >= 2, (name, k)
    # the bf16 32x32x16 kernel for 6 and for 9 products + the 16x16x32 fp16 kernel and its many-item form + the two-operand
    # GEMM's store form (three products), its one-product sum-of-squares form and its two-product dot form (AWQ searches)
    # and its many-problem form
    assert seen == 8


@needs_hipcc
def test_gptq_loop_kernels_do_not_spill():
    """`gptq_rows16_kernel` is launched with up to 1024 threads (<= 128 registers) and is a chain of dependent instructions:
    twice during its writing the optimiser produced 140 spilled registers (updates of later slabs sunk to the end of the
    slab; all 16 steps' LDS reads hoisted) without any functional test noticing.  `panel_update_kernel` needs two blocks per
    CU (64 KB of LDS each)."""
    seen = report("gptq_loop.hip").kernels
    rows16 = next(v for k, v in seen.items() if "gptq_rows16_kernel" in k)
    panel = next(v for k, v in seen.items() if "panel_update_kernel" in k)
    assert rows16.vgprs <= 128 and rows16.scratch == 0 and rows16.lds <= 65536, rows16
    assert panel.scratch == 0 and panel.occupancy >= 2 and panel.lds <= 65536, panel


@needs_hipcc
def test_resident_rtn_kernels_keep_their_tiles_in_registers():
    """`rtn_resident_groups` (channel, tall groups: W read once) holds a 128 x 256 tile in 64 registers per lane while the range
    completes elsewhere; two 8-wave workgroups per CU (<= 128 registers, no scratch) are what keeps loads in flight while one of
    them waits.  `rtn_resident_stream` holds two such tiles per workgroup, one 8-wave workgroup per CU (<= 256 registers, no
    scratch, two waves per SIMD).  `rtn_tensor_onepass` runs ONE 8-wave workgroup per CU that keeps a tile in 64 architectural registers, two in
    its 128 accumulation registers -- named as PHYSICAL registers a[0..127] in the assembly text, so the register allocator
    must not have placed anything of its own there -- and one in LDS; a spill would turn its kept tiles into scratch traffic."""
    seen, asm = report("rtn_resident.hip")
    for key, max_vgprs, min_occ in (("rtn_resident_groups", 128, 4), ("rtn_resident_stream", 256, 2), ("rtn_tensor_onepass", 256, 2)):
        hits = [v for k, v in seen.items() if key in k]
        assert hits, (key, list(seen))
        for k in hits:
            assert k.vgprs <= max_vgprs and k.scratch == 0 and k.occupancy >= min_occ, (key, k)
    # the per-tensor kernel's parks: the code object holds exactly the accumulation-register traffic the source writes (two parks
    # of 64 registers, each written at one place and read back at one place) and no other use of an `a` register: the compiler
    # turns to them only once the architectural registers run out (<= 128 here), and then it would take a[0], a[1], ... -- the parks
    with open(asm) as f:
        text = f.read()
    m = re.search(r"^_ZN2oq18rtn_tensor_onepassENS_12ResidentArgsE:.*?s_endpgm", text, re.S | re.M)
    assert m, "kernel body not found"
    body = m.group(0)
    writes = re.findall(r"v_accvgpr_write_b32 (\S+),", body)
    reads = re.findall(r"v_accvgpr_read_b32 \S+, (\S+)", body)
    assert len(writes) == 128 and len(reads) == 128 and len(set(writes)) == 128 and len(set(reads)) == 128, (len(writes), len(reads))
    assert all(w.startswith("a[") for w in writes) and all(r.startswith("a[") for r in reads), "an accumulation register the source did not name"
    assert "v_accvgpr_mov" not in body
    others = [ln for ln in body.splitlines() if "accvgpr" not in ln and re.search(r"[ ,]a(\[|\d)", ln.split(";")[0])]
    assert not others, others[:5]
    meta = [c for c in text.split("- .agpr_count:")[1:] if "_ZN2oq18rtn_tensor_onepassENS_12ResidentArgsE\n" in c.split(".vgpr_count:")[0]]
    assert len(meta) == 1
    agpr = int(meta[0].split()[0])
    total = int(re.search(r"\.vgpr_count:\s+(\d+)", meta[0]).group(1))
    assert agpr == 128 and total <= 256, (agpr, total)      # the descriptor reserves a[0..127]; with the architectural ones: two waves per SIMD


@needs_hipcc
@pytest.mark.parametrize("source,kernels", [("rtn_mse.hip", ("mse_rows_reg_kernel",)), ("hqq.hip", ("hqq_rounds_reg_kernel",)),
                                            ("awq.hip", ("awq_group_diff_kernel",))])
def test_register_tile_search_kernels_do_not_spill(source, kernels):
    """(awq.hip: the quantize-residual kernel keeps a block's rows in registers from the load to the difference and, since round 5,
    through the packing of the loss product's fp16 pieces.)
    The MSE and HQQ searches hold a group's G values in registers across all candidates / rounds.  Left to itself the
    optimiser interleaves independent chunks until the G = 128 tile spills (1.1 KB of scratch per lane and 3x the time, with
    every parity test still green): the chunks are chained through opaque copies and this test watches the result."""
    seen = report(source).kernels
    for key in kernels:
        hits = {k: v for k, v in seen.items() if key in k}
        assert hits, (key, list(seen))
        for name, k in hits.items():
            assert k.scratch == 0 and k.occupancy >= 2, (name, k)
