"""The kernels of csrc/rtn_mse.hip for every element type, from the compiler's own resource report (hipcc cross-compiles
without a GPU).  mse_rows_reg_kernel holds a group's values in registers across the 20 candidates: fp32 as they are, fp16 / bf16
converted at the load for groups of up to 128, and PACKED two per register for groups of 256 (which exist for the 2-byte types
only).  A spilled tile keeps every parity test green at a fraction of the speed, so: no scratch, no spill, and two waves per
SIMD at least.  Resource figures only; no figure of a particular compiler is written down here."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FP32_GROUPS = (32, 64, 128)
HALF_GROUPS = (32, 64, 128, 256)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_mse_register_tiles_of_every_element_type_do_not_spill(tmp_path):
    from onnx_quantize_amd import _build
    src = os.path.join(ROOT, "onnx_quantize_amd", "csrc", "rtn_mse.hip")
    r = subprocess.run([HIPCC, *_build.flags_for(src), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o",
                        str(tmp_path / "rtn_mse.s"), src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                         r"SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", r.stderr, re.S):
        seen[m.group(1)] = tuple(int(m.group(i)) for i in (2, 3, 4, 5, 6))
    tiles = {k: v for k, v in seen.items() if "mse_rows_reg_kernel" in k}

    def built(elem):
        """Group sizes instantiated for an element type, from the mangled template arguments <oq::Elem, G>."""
        return sorted(int(m.group(1)) for m in (re.search(r"mse_rows_reg_kernelINS_\d+%sELi(\d+)E" % elem, k) for k in tiles) if m)

    assert built("MseF32") == list(FP32_GROUPS), sorted(tiles)                     # still three: no fp32 tile of 256
    assert built("ElemF16") == built("ElemBF16") == list(HALF_GROUPS), sorted(tiles)
    assert len(tiles) == len(FP32_GROUPS) + 2 * len(HALF_GROUPS), sorted(tiles)
    for name, (vgprs, scratch, occ, sgpr_spill, vgpr_spill) in tiles.items():
        assert scratch == 0 and sgpr_spill == 0 and vgpr_spill == 0, (name, vgprs, scratch, sgpr_spill, vgpr_spill)
        assert occ >= 2, (name, vgprs, occ)
    for key in ("mse_rows_kernel", "mse_tensor_partial", "tensor_minmax_kernel"):  # fp32, fp16, bf16
        assert sum(key in k for k in seen) == 3, (key, sorted(seen))
    for key in ("mse_tensor_mask", "mse_resolve_kernel"):                          # they never see W
        assert sum(key in k for k in seen) == 1, (key, sorted(seen))
