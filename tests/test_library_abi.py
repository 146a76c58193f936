"""The C-ABI library: builds for gfx950 without a GPU, loads, and exports exactly the symbols that
include/oq_hip.h declares and the ctypes stub binds.  No compute call is made here (CPU-only suite)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "oq_hip.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(oq_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib_path():
    from onnx_quantize_amd import _build
    return _build.build(verbose=False)


def test_header_matches_ctypes_prototypes():
    from onnx_quantize_amd.hip import _lib
    assert declared_symbols() == sorted(_lib.PROTOTYPES)


def test_library_exports_every_declared_symbol(lib_path):
    lib = ctypes.CDLL(lib_path)
    for name in declared_symbols():
        assert hasattr(lib, name), f"{name} is declared in include/oq_hip.h but not exported"
    lib.oq_target_arch.restype = ctypes.c_char_p
    assert lib.oq_target_arch() == b"gfx950"
    assert lib.oq_abi_version() == 2


def test_code_object_is_gfx950(lib_path, tmp_path):
    # llvm-objdump --offloading drops the extracted code objects next to its input: work on a copy outside the tree
    import shutil
    copy = shutil.copy(lib_path, tmp_path / "liboq_hip.so")
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", str(copy)], capture_output=True, text=True,
                         cwd=tmp_path)
    assert "gfx950" in out.stdout + out.stderr


def test_header_is_plain_c_and_links(lib_path, tmp_path):
    """tests/c/abi_check.c: include/oq_hip.h compiles as C99, every declared entry point resolves against the library
    and the host-only calls answer; the list of symbols in the C file must be the header's."""
    src = os.path.join(ROOT, "tests", "c", "abi_check.c")
    text = open(src).read()
    assert sorted(set(re.findall(r"TAKE\((oq_[a-z0-9_]+)\)", text))) == declared_symbols()
    exe = tmp_path / "abi_check"
    libdir = os.path.dirname(lib_path)
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", str(exe),
                         "-L", libdir, "-loq_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(os.path.dirname(torch.__file__), "lib"), "/opt/rocm/lib",
                                               env.get("LD_LIBRARY_PATH", "")])
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stdout.startswith("ok "), (run.returncode, run.stdout, run.stderr)


def test_host_only_entry_points(lib_path):
    """oq_qrange / status strings / argument validation run on the host and need no device."""
    from onnx_quantize_amd.hip import _lib
    lib = _lib.load()
    assert _lib.qrange(_lib.OQ_INT4, True, False) == (-7, 7)
    assert _lib.qrange(_lib.OQ_UINT8, True, True) == (0, 127)
    assert _lib.qrange(_lib.OQ_INT32, False, False) == (-2**31, 2**31 - 1)
    assert lib.oq_status_string(-3) == b"workspace too small"
    with pytest.raises(_lib.OqHipError, match="unknown quantization type"):
        _lib.qrange(17, False, False)
    # null pointers are rejected before any launch
    st = lib.oq_rtn_quantize_f32(None, 4, 4, 4, 0, 0, -1, 0, 0, 1.0, 0, None, None, None, 0, None, 0, None)
    assert st == -1 and b"null pointer" in lib.oq_last_error()
    assert lib.oq_rtn_workspace_bytes(4096, 11008, _lib.OQ_GROUP, 128, 0) > 0
    # the batched factor: workspace grows linearly with the batch, bad batches are refused before any launch
    one, four = lib.oq_gptq_factor_workspace_bytes(4096), lib.oq_gptq_factor_batched_workspace_bytes(4096, 4)
    # (the operand pieces of the inverse levels add per-call tables and paddings: linear up to a few KB)
    assert lib.oq_gptq_factor_batched_workspace_bytes(4096, 1) == one and abs(four - 4 * one) < 16384
    assert lib.oq_gptq_factor_batched_workspace_bytes(4096, 0) == 0
    import ctypes as C
    dummy = (C.c_float * 4)()
    info = (C.c_int32 * 4)()
    for count, stride, needle in ((0, 16, b"bad argument"), (70000, 16, b"bad argument"), (2, 8, b"overlap")):
        st = lib.oq_gptq_factor_batched_f32(dummy, 4, stride, count, 0.01, 0, dummy, stride, info, 0, dummy, 16, None)
        assert st == -1 and needle in lib.oq_last_error(), (count, stride, lib.oq_last_error())
    st = lib.oq_gptq_factor_batched_f32(dummy, 4, 16, 2, 0.01, 0, dummy, 16, info, 0, dummy, 16, None)
    assert st == -3 and b"workspace" in lib.oq_last_error()
    # ABI 2: the method is an argument (no process-wide setter is exported any more); unknown values are refused per call
    assert not hasattr(lib, "oq_hessian_set_method") and not hasattr(lib, "oq_hessian_method")
    st = lib.oq_gptq_factor_batched_f32(dummy, 4, 16, 2, 0.01, 0, dummy, 16, info, 7, dummy, 16, None)
    assert st == -1 and b"unknown method" in lib.oq_last_error()
    st = lib.oq_hessian_accumulate_f32(dummy, 4, 4, 4, 0, 1, dummy, 9, None, 0, None)
    assert st == -1 and b"unknown method" in lib.oq_last_error()


def test_missing_library_is_loud(monkeypatch, tmp_path):
    from onnx_quantize_amd.hip import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.OqHipMissing, match="no CPU fallback"):
        _lib.load()


def test_ops_refuse_host_tensors():
    import torch
    from onnx_quantize_amd.hip import ops
    with pytest.raises(TypeError, match="no CPU fallback"):
        ops.rtn_quantize(torch.zeros(4, 4), "int8", "tensor")
    with pytest.raises(TypeError):
        ops.minmax_collect(torch.zeros(4), torch.zeros(4), 0.0)


def _fnv1a(b: bytes) -> int:
    h = 1469598103934665603
    for byte in b:
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.gpu
def test_c_program_quantizes_on_the_gpu(tmp_path):
    """The boundary is a C ABI, not a torch extension: a C99 program that links liboq_hip.so and the HIP runtime only
    (tests/c/rtn_direct.c) quantizes a matrix on the GPU; its output digests equal the oracle's on the same data, its
    error path returns a status and a text."""
    import shutil
    import subprocess
    import numpy as np
    from oracle import oq_oracle as O
    from onnx_quantize_amd import _build

    gcc, rocm = shutil.which("gcc"), "/opt/rocm"
    if gcc is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("gcc or the ROCm headers are not on this box")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "rtn_direct")
    lib_dir = os.path.dirname(_build.LIB)
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(root, "include"),
                    "-I", os.path.join(rocm, "include"), os.path.join(root, "tests", "c", "rtn_direct.c"), "-L", lib_dir, "-loq_hip",
                    "-L", os.path.join(rocm, "lib"), "-lamdhip64", f"-Wl,-rpath,{lib_dir}", f"-Wl,-rpath,{rocm}/lib", "-o", exe],
                   check=True, capture_output=True, text=True)
    k, n = 512, 384
    out = subprocess.run([exe, str(k), str(n)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    # the same LCG as the C program
    x, vals = 12345, np.empty(k * n, np.float32)
    state = np.uint32(x)
    seq = np.empty(k * n, np.uint32)
    with np.errstate(over="ignore"):
        for i in range(k * n):
            state = np.uint32(state * np.uint32(1664525) + np.uint32(1013904223))
            seq[i] = state
    vals = ((seq >> np.uint32(8)).astype(np.float32) / np.float32(16777216.0) - np.float32(0.5)) * np.float32(4.0)
    w = vals.reshape(k, n)
    q, s, z = O.rtn_quantize(w, "uint4", "group", 128)
    blob, _, _ = O.matmul_nbits_layout(q, s, z, 128, 4)
    kn = dict(item.split("=") for item in out[0].split()[1:])
    assert int(kn["q"], 16) == _fnv1a(q.tobytes()) and int(kn["scale"], 16) == _fnv1a(np.ascontiguousarray(s, np.float32).tobytes())
    assert int(kn["zp"], 16) == _fnv1a(np.ascontiguousarray(z, np.uint8).tobytes())
    assert int(out[1].split("=")[1], 16) == _fnv1a(blob.tobytes())
    assert out[2].startswith("error status=-2") and "NBITS layout needs the group strategy" in out[2]


def test_shipped_library_has_no_attribution_switches():
    """The shipped library has no experiment switches at all: no file of its sources so much as mentions `getenv` (not even
    behind an `#ifdef` or in a comment), the lab macros that once selected or tuned variants of the Hessian / piece-GEMM and AWQ
    kernels are gone with the variants, the store-dropping RTN variants and the `nt` argument that selected them are gone, the
    switches and phase stamps of the ticketed RTN kernels and of the GPTQ loop are gone (the only preprocessor conditional on an
    `OQ_` macro left is `OQ_SPIN_LIMIT`), and the build used by `__graft_entry__.build()` and the tests defines no lab macro."""
    from onnx_quantize_amd import _build
    removed_macros = ("OQ_SYRK_LAB", "OQ_SYRK_F16_M16", "OQ_SYRK_SPLITS", "OQ_SYRK_F16_STRIDE", "OQ_SYRK_F16_STRIDE_EXPR", "OQ_SYRK_F16_DEEP",
                      "OQ_SYRK_M16_STRIDE", "OQ_PREP_NT", "OQ_PREP_LOAD", "OQ_AWQ_HI_ONLY", "OQ_AWQ_FUSED_PIECES", "OQ_AWQ_GRAM_RATIO",
                      "OQ_RES_A_NT", "OQ_RES_SLEEP", "OQ_RES_STORE", "OQ_GROUPS_GROUP", "OQ_STREAM_GROUP", "OQ_T4_GROUP", "OQ_TENSOR_STAMPS",
                      "OQ_NO_TICKET_CHAIN", "OQ_LOOP_STAMPS")
    conditionals = []
    for name in sorted(os.listdir(_build.SRC)):
        text = open(os.path.join(_build.SRC, name)).read()
        assert "getenv" not in text, name
        for macro in removed_macros:
            assert macro not in text, (name, macro)
        assert "OQ_RTN_ATTRIBUTION" not in text and "OQ_ATTR(" not in text, name
        assert not re.search(r"\ba\.nt\b", text), name       # the field itself (`a.ntiles` of the ticketed kernels is another thing)
        assert not re.search(r"\bOQ_(STAMP|LAP)\b", text), name     # the phase stamps of the ticketed kernels and of the GPTQ loop
        conditionals += re.findall(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b[^\n]*?\b(OQ_\w+)", text, re.M)
    # the one switch left: spins that give up instead of hanging a shared box, for the first runs of a changed hand-off
    assert conditionals and set(conditionals) == {"OQ_SPIN_LIMIT"}, conditionals
    for flag in _build.CXXFLAGS + [f for fl in _build.PER_FILE_FLAGS.values() for f in fl]:
        assert not re.match(r"-D\s*\w*_LAB\b", flag) and "OQ_RTN_ATTRIBUTION" not in flag, flag


def test_element_types_live_in_one_header():
    """csrc/half_elem.hpp is the one place that knows the element types of W and X: no other source defines an
    element struct (a `typedef ... raw;` inside a `struct`), none names the element by a `bool BF16` template parameter or through
    the `HalfElem<>` adapter that served those, and none compares a runtime value with OQ_W_F16 / OQ_W_BF16 (`==`, `!=`, `?`):
    a type code becomes an element type in `with_half_elem` only."""
    from onnx_quantize_amd import _build
    code = r"\bOQ_W_B?F16\b"
    compared = re.compile(r"(?:==|!=)\s*%s|%s\s*(?:==|!=|\?)|\?[^;\n]*%s" % (code, code, code))
    header = open(os.path.join(_build.SRC, "half_elem.hpp")).read()
    assert len(re.findall(r"struct\s+\w+\s*\{[^}]*?typedef[^;}]*\braw\s*;", header)) == 3 and compared.search(header)     # the patterns see what they look for
    for name in sorted(os.listdir(_build.SRC)):
        if name == "half_elem.hpp":
            continue
        text = open(os.path.join(_build.SRC, name)).read()
        assert not re.search(r"struct\s+\w+\s*\{[^}]*?typedef[^;}]*\braw\s*;", text), name
        assert "HalfElem<" not in text and not re.search(r"template\s*<[^>]*\bbool\s+BF16\b", text), name
        assert not compared.search(text), (name, compared.search(text).group(0))


@pytest.mark.gpu
def test_environment_knobs_cannot_change_the_bytes():
    """one stray environment variable (OQ_RTN_NT=56 dropped the parameter and blob stores in round 2) must not
    make liboq_hip.so return anything but the reference's bytes.  A fresh process (the knobs are read once) quantizes the
    KAT2 matrix with every output-relevant knob set to a hostile value and must still produce the reference's digests."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import hashlib, json, numpy as np, torch
from onnx_quantize_amd.hip import ops
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]
w = torch.from_numpy(np.random.default_rng(0).standard_normal((4096, 11008), dtype=np.float32)).cuda()
out = {}
blob, s, z = ops.rtn_quantize(w, "uint4", "group", 128, layout="nbits")
b = blob.cpu().numpy()
full = np.empty((11008, 32, 128), np.uint8); full[..., 0::2] = b & 0x0F; full[..., 1::2] = b >> 4
out["nbits"] = [sha(full.reshape(11008, 4096).T), sha(s.cpu().numpy()), sha(z.cpu().numpy())]
q, s, z = ops.rtn_quantize(w, "uint4", "group", 128, layout="kn")
out["kn"] = [sha(q.cpu().numpy()), sha(s.cpu().numpy()), sha(z.cpu().numpy())]
for strategy in ("channel", "tensor"):      # the ticketed kernels: OQ_RTN_RES_TILE picks among three of them, OQ_RTN_RESIDENT=0 the three-launch path
    q, s, z = ops.rtn_quantize(w, "int8", strategy, -1)
    out[strategy] = [sha(q.cpu().numpy()), sha(s.cpu().numpy()), sha(z.cpu().numpy())]
# the GPTQ path: Hessian, factor, corrected loop (VERDICT r03 item 7: OQ_HESSIAN_METHOD / OQ_GPTQ_ROWS16 / OQ_SYRK_F16_M16 used to
# be read by the shipped library; they must now change nothing)
g = torch.Generator(device="cuda").manual_seed(3)
x = torch.randn((4, 512, 1024), generator=g, device="cuda") * (1 + torch.arange(1024, device="cuda") % 7)
wg = torch.randn((1024, 256), generator=g, device="cuda") * 0.05
h = torch.zeros((1024, 1024), device="cuda")
ops.hessian_accumulate(x, h, 0)
q, s, z, _ = ops.gptq_quantize(wg, h, "int4", "group", 128, mode="corrected")
out["gptq"] = [sha(h.cpu().numpy()), sha(q.cpu().numpy()), sha(s.cpu().numpy()), sha(z.cpu().numpy())]
print(json.dumps(out))
'''
    with open(os.path.join(root, "tests", "golden", "digests.json")) as f:
        dall = json.load(f)
    d = dall["config2_asym"]
    expect = [d["q_sha"], d["s_sha"], d["z_sha"]]
    expect_rng = {st: [dall[f"headline_int8_{st}"][k] for k in ("q_sha", "s_sha", "z_sha")] for st in ("channel", "tensor")}
    gptq_bytes = None
    hostile = [dict(OQ_RTN_NT="56"), dict(OQ_RTN_NT="127"), dict(OQ_RTN_NT="120", OQ_RTN_RESIDENT="0", OQ_RTN_RES_TILE="32"),
               dict(OQ_HESSIAN_METHOD="1", OQ_GPTQ_ROWS16="0", OQ_SYRK_F16_M16="0", OQ_SYRK_SPLITS="1"), dict(OQ_RTN_RES_TILE="1"),
               dict(OQ_RTN_RES_TILE="128", OQ_RES_SLEEP="0"), dict(OQ_RTN_RES_TILE="256", OQ_AWQ_GRAM_RATIO="1"), dict()]
    for knobs in hostile:
        clean = {k: v for k, v in os.environ.items() if not k.startswith("OQ_")}
        env = dict(clean, PYTHONPATH=root, **knobs)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        got = json.loads(r.stdout.strip().splitlines()[-1])
        assert got["nbits"] == expect and got["kn"] == expect, (knobs, got)
        assert got["channel"] == expect_rng["channel"] and got["tensor"] == expect_rng["tensor"], (knobs, got)
        gptq_bytes = gptq_bytes or got["gptq"]
        assert got["gptq"] == gptq_bytes, (knobs, got["gptq"], gptq_bytes)     # Hessian, integers, scales, zero points: the same bits
