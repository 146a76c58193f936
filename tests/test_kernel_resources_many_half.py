"""The table forms of the fused half RTN kernels (csrc/rtn_half.hip: rtn_half_wave_many, rtn_half_column_many) against their
single-matrix twins, from the compiler's own resource report (hipcc cross-compiles without a GPU).

Both forms run ONE __device__ body; the table form adds four scalar loads and the [K, N/2] epilogue.  The 16-row build with
16-byte loads sits right at the boundary of three waves per SIMD (docs/LAB_NOTES_r07.md), so neither addition may cost a wave or
scratch traffic there.  The kernels are compared with each other: no figure of a particular compiler is written down here."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_table_kernels_keep_the_occupancy_of_their_single_matrix_twins(tmp_path):
    from onnx_quantize_amd import _build
    src = os.path.join(ROOT, "onnx_quantize_amd", "csrc", "rtn_half.hip")
    r = subprocess.run([HIPCC, *_build.flags_for(src), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o",
                        str(tmp_path / "rtn_half.s"), src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", r.stderr, re.S):
        seen[m.group(1)] = (int(m.group(2)), int(m.group(3)))            # (scratch, occupancy)
    pairs = []
    for elem in ("NS_7ElemF16E", "NS_8ElemBF16E"):
        for rows in (16, 32):
            for vec in (1, 0):
                build = f"I{elem}Li{rows}ELb{vec}EEEv"
                pairs.append((rows == 16 and vec == 1, f"_ZN2oq13rtn_half_wave{build}NS_8HalfArgsE",
                              f"_ZN2oq18rtn_half_wave_many{build}NS_8HalfArgsEPKNS_8HalfPtrsE"))
        pairs.append((False, f"_ZN2oq15rtn_half_columnI{elem}EEvNS_8HalfArgsE", f"_ZN2oq20rtn_half_column_manyI{elem}EEvNS_8HalfArgsEPKNS_8HalfPtrsE"))
    assert len(pairs) == 10
    for hot, single, many in pairs:
        assert single in seen and many in seen, (single, many, sorted(seen))
        (s_scratch, s_occ), (m_scratch, m_occ) = seen[single], seen[many]
        if hot:       # the 16-row build with 16-byte loads: the occupancy of the twin and no more scratch than it
            assert m_occ == s_occ and m_scratch <= s_scratch, (many, seen[many], seen[single])
        else:         # every other build: no scratch where the twin has none
            assert m_scratch == 0 or s_scratch > 0, (many, seen[many], seen[single])
