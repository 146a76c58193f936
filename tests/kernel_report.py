"""The compiler's own resource report of a HIP source, for the tests that guard registers, scratch and occupancy (hipcc
cross-compiles without a GPU).  `report(source)` compiles csrc/<source> once per test process, with the flags the library is
built with, and returns the figures per mangled kernel name and the path of the assembly text."""
import atexit
import collections
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

# one entry of -Rpass-analysis=kernel-resource-usage; `agprs` is None where the compiler prints none
Kernel = collections.namedtuple("Kernel", "vgprs agprs scratch occupancy sgpr_spill vgpr_spill lds")
Report = collections.namedtuple("Report", "kernels asm")       # {mangled name: Kernel}, path of the .s file

_FIELDS = (("vgprs", r" VGPRs: (\d+)"), ("agprs", r" AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
           ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"),
           ("lds", r"LDS Size \[bytes/block\]: (\d+)"))
ALL_ELEMS, HALF_ELEMS = ["ElemBF16", "ElemF16", "ElemF32"], ["ElemBF16", "ElemF16"]      # csrc/half_elem.hpp, sorted
_out_dir = None


def element_types(kernels, name: str) -> list:
    """The element types the kernel template `name`<E> or `name`<E, ...> is instantiated for, sorted, from the mangled names."""
    return sorted(m.group(1) for m in (re.search(r"\d+%sINS_\d+(Elem\w+?)E[EL]" % name, k) for k in kernels) if m)


@functools.lru_cache(maxsize=None)
def report(source: str) -> Report:
    from onnx_quantize_amd import _build
    global _out_dir
    if _out_dir is None:
        _out_dir = tempfile.mkdtemp(prefix="oq_kernel_report_")
        atexit.register(shutil.rmtree, _out_dir, ignore_errors=True)
    src = os.path.join(ROOT, "onnx_quantize_amd", "csrc", source)
    asm = os.path.join(_out_dir, source[:-4] + ".s")
    r = subprocess.run([HIPCC, *_build.flags_for(src), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", asm, src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = {}
    for entry in r.stderr.split("Function Name: ")[1:]:
        values = {}
        for field, pattern in _FIELDS:
            m = re.search(pattern, entry)
            assert m or field == "agprs", (field, entry[:400])
            values[field] = int(m.group(1)) if m else None
        kernels[entry.split()[0]] = Kernel(**values)
    assert kernels, r.stderr[-2000:]
    return Report(kernels, asm)
