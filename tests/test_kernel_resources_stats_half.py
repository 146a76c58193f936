"""The kernels of csrc/abs_stats_half.hip (oq_abs_stats_cols_many_h16) from the compiler's own resource report (hipcc
cross-compiles without a GPU): HBM-bound streams that keep 8 or 16 row loads in flight per lane, so scratch traffic would compete
with the stream itself.  No figure of a particular compiler is written down here: no scratch, no spill, and a 256-thread block
must fit a SIMD's share of the registers at all."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_abs_stats_kernels_have_no_scratch(tmp_path):
    from onnx_quantize_amd import _build
    src = os.path.join(ROOT, "onnx_quantize_amd", "csrc", "abs_stats_half.hip")
    r = subprocess.run([HIPCC, *_build.flags_for(src), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o",
                        str(tmp_path / "abs_stats_half.s"), src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                         r"SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", r.stderr, re.S):
        seen[m.group(1)] = tuple(int(m.group(i)) for i in (2, 3, 4, 5))
    for key, copies in (("abs_stats_half_partial", 2), ("abs_stats_half_fold", 1)):          # fp16 and bf16 instantiations
        assert sum(key in name for name in seen) == copies, (key, list(seen))
    assert len(seen) == 3, list(seen)
    for name, (scratch, occ, sgpr_spill, vgpr_spill) in seen.items():
        assert scratch == 0 and sgpr_spill == 0 and vgpr_spill == 0, (name, scratch, sgpr_spill, vgpr_spill)
        assert occ >= 1, (name, occ)
    asm = open(tmp_path / "abs_stats_half.s").read()
    assert "flat_load" not in asm and "flat_store" not in asm              # table pointers are used as global memory
