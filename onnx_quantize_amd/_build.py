"""Build liboq_hip.so (the C-ABI HIP library) in-tree with hipcc for gfx950.

    python -m onnx_quantize_amd._build          # incremental
    python -m onnx_quantize_amd._build --force

hipcc cross-compiles without a GPU.  Objects go to ``build/`` (git-ignored), the shared
library to ``onnx_quantize_amd/lib/liboq_hip.so`` (git-ignored, but it travels with the
repo snapshot to the GPU box).
"""
from __future__ import annotations

import concurrent.futures
import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
SRC = os.path.join(PKG, "csrc")
OBJ = os.path.join(ROOT, "build", "oq_hip")
LIB_DIR = os.path.join(PKG, "lib")
LIB = os.path.join(LIB_DIR, "liboq_hip.so")
ARCH = "gfx950"

# -ffp-contract=off: the reference rounds every product/sum separately (SURVEY.md finding 3);
# no fast-math anywhere: fp32 division must stay IEEE (utils.py:73).
CXXFLAGS = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
            "-fno-fast-math", "-Wall", "-Wno-unused-function"]


# Per-file additions.  hqq.hip: the SLP vectoriser pairs the register tile's values for v_pk_mul / v_pk_add; the aligned
# register pairs fragment the allocation until the G = 128 tile of hqq_rounds_reg_kernel spills (256 registers + scratch against
# 165 registers without pairing; tests/test_kernel_resources.py watches it).
# matmul_nbits.hip: paired, the per-group fold `sum = fma(acc, scale, sum)` of tile_gemm (csrc/nbits_tile.hpp) becomes v_pk_fma_f32 with
# an op_sel on the scale pair, and on the MI355X those gave wrong low halves in lanes 48 .. 63 whenever several waves shared a SIMD
# (docs/LAB_NOTES_r22.md; tests/test_matmul_nbits_gpu.py holds exact products on large grids against it, and
# tests/test_qdq_matmul_resources.py finds no v_pk_fma_f32 in the file's assembly).
# matmul_nbits_decode.hip: the same fold, sum = fma(acc, scale, sum), on the vector ALU throughout: built unpaired from its first compile
# (tests/test_matmul_nbits_decode_resources.py finds no v_pk_fma_f32 in its assembly).
# qdq_matmul.hip: the tile kernel of matmul_nbits.hip on a [K, N] byte matrix, the same fold: unpaired from its first compile too
# (tests/test_qdq_matmul_resources.py).
# matmul_nbits_fzp.hip: tile_gemm once more, with a second scalar fma in the fold (the float zero point's correction): unpaired from its
# first compile (tests/test_matmul_nbits_fzp_resources.py).
PER_FILE_FLAGS = {"hqq.hip": ("-fno-slp-vectorize",), "matmul_nbits.hip": ("-fno-slp-vectorize",),
                  "matmul_nbits_decode.hip": ("-fno-slp-vectorize",), "qdq_matmul.hip": ("-fno-slp-vectorize",),
                  "matmul_nbits_fzp.hip": ("-fno-slp-vectorize",)}


def flags_for(src: str) -> list[str]:
    return [*CXXFLAGS, *PER_FILE_FLAGS.get(os.path.basename(src), ())]


def hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the HIP library cannot be built")
    return exe


def sources() -> list[str]:
    return sorted(os.path.join(SRC, f) for f in os.listdir(SRC) if f.endswith(".hip"))


def _deps_mtime() -> float:
    hdrs = [os.path.join(SRC, f) for f in os.listdir(SRC) if f.endswith((".hpp", ".h"))]
    hdrs.extend(os.path.join(ROOT, "include", h) for h in ("oq_hip.h", "oq_hip_half.h", "oq_hip_nbits.h", "oq_hip_nbits_decode.h", "oq_hip_nbits_fzp.h", "oq_hip_qlinear.h",
                                                           "oq_hip_qlinear_decode.h", "oq_hip_qlinear_function.h", "oq_hip_qdq.h", "oq_hip_qdq_function.h"))
    return max(os.path.getmtime(h) for h in hdrs)


def _compile(src: str, force: bool, extra: tuple = ()) -> str:
    obj = os.path.join(OBJ, os.path.basename(src)[:-4] + ".o")
    newest = max(os.path.getmtime(src), _deps_mtime())
    if not force and os.path.exists(obj) and os.path.getmtime(obj) >= newest:
        return obj
    cmd = [hipcc(), *flags_for(src), *extra, "-c", src, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
    if r.stderr.strip():
        sys.stderr.write(r.stderr)
    return obj


def build(force: bool = False, verbose: bool = True, extra_flags: tuple = ()) -> str:
    """``extra_flags`` is for lab builds only (``--define`` below); `__graft_entry__.build()` and the tests never pass any."""
    os.makedirs(OBJ, exist_ok=True)
    os.makedirs(LIB_DIR, exist_ok=True)
    srcs = sources()
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(6, len(srcs))) as ex:
        objs = list(ex.map(lambda s: _compile(s, force, tuple(extra_flags)), srcs))
    if force or not os.path.exists(LIB) or any(os.path.getmtime(o) > os.path.getmtime(LIB) for o in objs):
        cmd = [hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB, *objs]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
        if verbose:
            print(f"[oq build] linked {LIB}")
    elif verbose:
        print(f"[oq build] up to date: {LIB}")
    return LIB


if __name__ == "__main__":
    if "--define" in sys.argv:               # lab builds on a GPU box's scratch copy: --define NAME [--define NAME ...]
        build(force=True, extra_flags=tuple("-D" + sys.argv[i + 1] for i, a in enumerate(sys.argv[:-1]) if a == "--define"))
    else:
        build(force="--force" in sys.argv)
