"""The kernels of csrc/awq.hip that read W, for every element type, from the compiler's own resource report (hipcc cross-compiles
without a GPU).  awq_group_diff_kernel holds a lane's 16 rows x 4 columns in registers from the load to the difference and runs
512 threads at two waves per SIMD; fp32 loads them as 16 float4, fp16 / bf16 as 16 words of 8 bytes converted at the load.  A
spilled tile keeps every parity test green at a fraction of the speed, so: no scratch, no spill, and two waves per SIMD at least,
for every instantiation.  Resource figures only; no figure of a particular compiler is written down here."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ELEMS = ("AwqF32", "ElemF16", "ElemBF16")
TEMPLATED = ("group_absmax_kernel", "weight_scale_rows_kernel", "row_absmax_kernel", "scale_rows_kernel", "awq_diff_kernel", "awq_diff4_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_awq_kernels_of_every_element_type_do_not_spill(tmp_path):
    from onnx_quantize_amd import _build
    src = os.path.join(ROOT, "onnx_quantize_amd", "csrc", "awq.hip")
    r = subprocess.run([HIPCC, *_build.flags_for(src), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o",
                        str(tmp_path / "awq.s"), src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                         r"SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", r.stderr, re.S):
        seen[m.group(1)] = tuple(int(m.group(i)) for i in (2, 3, 4, 5, 6))

    # the fused quantize-residual kernel: <element, PIECES> for three elements and both values of PIECES
    fused = {k: v for k, v in seen.items() if "awq_group_diff_kernel" in k}
    built = sorted((e, p) for k in fused for e in ELEMS for p in (0, 1) if re.search(r"awq_group_diff_kernelINS_\d+%sELb%dE" % (e, p), k))
    assert built == sorted((e, p) for e in ELEMS for p in (0, 1)), sorted(fused)
    assert len(fused) == 6, sorted(fused)
    for name, (vgprs, scratch, occ, sgpr_spill, vgpr_spill) in fused.items():
        assert scratch == 0 and sgpr_spill == 0 and vgpr_spill == 0, (name, vgprs, scratch, sgpr_spill, vgpr_spill)
        assert occ >= 2, (name, vgprs, occ)

    # every other kernel that reads W: fp32, fp16, bf16, none of them with scratch
    for key in TEMPLATED:
        mine = {k: v for k, v in seen.items() if re.search(r"\d+%sINS_" % key, k)}
        assert sorted(e for k in mine for e in ELEMS if re.search(r"%sINS_\d+%sEE" % (key, e), k)) == sorted(ELEMS), (key, sorted(mine))
        for name, (vgprs, scratch, occ, sgpr_spill, vgpr_spill) in mine.items():
            assert scratch == 0 and sgpr_spill == 0 and vgpr_spill == 0, (name, vgprs, scratch, sgpr_spill, vgpr_spill)
