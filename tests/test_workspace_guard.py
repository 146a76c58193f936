"""CPU guards for the layout of caller-provided workspaces.  A `*_workspace_bytes` query and the entry point it
belongs to run ONE layout function against csrc/workspace.hpp, so what the query promises is what the entry point carves.
tests/c/workspace_walk.cpp replays layouts of the library on heap blocks of exactly the measured size, built here with
AddressSanitizer and run on the host; the scans below keep hand-written alignment arithmetic and a second split-K plan out of
the sources."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "onnx_quantize_amd", "csrc")
WALK = os.path.join(ROOT, "tests", "c", "workspace_walk.cpp")


def _gxx():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    return gxx


def test_carved_pieces_stay_inside_a_workspace_of_the_measured_size_under_asan(tmp_path):
    exe = str(tmp_path / "workspace_walk")
    subprocess.run([_gxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, WALK, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "bad=0" in r.stdout


def test_the_guard_catches_a_measuring_run_without_its_pad(tmp_path):
    """The same program against a copy of the header whose measuring total leaves out the pad of an unaligned base -- a query that
    promises less than the entry point carves -- must die under ASan: otherwise the guard guards nothing."""
    src = open(os.path.join(CSRC, "workspace.hpp")).read()
    broken = src.replace("size_t total() const { return add(off_, pad_); }", "size_t total() const { return off_; }")
    assert broken != src
    inc = tmp_path / "inc"
    inc.mkdir()
    (inc / "workspace.hpp").write_text(broken)
    exe = str(tmp_path / "broken")
    subprocess.run([_gxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address", "-I", str(inc), WALK, "-o", exe], check=True, capture_output=True,
                   text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr


# rounding up to 256 by hand: `(x + 255) / 256 * 256` (a launch grid, `(n + 255) / 256` blocks of 256 threads, is not followed by `* 256`),
# `(x + 255) & ~255`, and the pad of a pointer, `(256 - p % 256) % 256` or `(256 - (p & 255)) & 255`
ROUND_UP = re.compile(r"\+\s*255u?\s*\)\s*/\s*256\s*\)*\s*\*\s*256|\+\s*255u?\s*\)\s*&\s*~")
POINTER_PAD = re.compile(r"%\s*256\s*\)\s*%\s*256|&\s*255u?\s*\)\s*\)\s*&\s*255")
ROUND_UP_NAME = re.compile(r"\balign256\b|\br256\b")
# the arithmetic of the split-K plan: how many ways K is split
SPLIT_PLAN = re.compile(r"min<int64_t>\(\s*8\s*,\s*steps\s*\)")


def _sources():
    return {name: open(os.path.join(CSRC, name)).read() for name in sorted(os.listdir(CSRC))}


def test_the_patterns_see_what_they_look_for():
    assert ROUND_UP.search("size_t r256(int64_t n) { return (static_cast<size_t>(n) + 255) / 256 * 256; }")
    assert ROUND_UP.search("return gemm_f16x3_pieces_bytes(Kd, cols) + ((static_cast<size_t>(cols) * 8 + 255) / 256) * 256;")
    assert ROUND_UP.search("base = reinterpret_cast<uint32_t*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~static_cast<uintptr_t>(255));")
    assert not ROUND_UP.search("hipLaunchKernelGGL(clear_words_kernel, dim3((n16 + 255) / 256), dim3(256), 0, s, p, n16);")
    assert not ROUND_UP.search("const dim3 grid(static_cast<uint32_t>((n + 255) / 256), 256 * 2);")
    assert POINTER_PAD.search("wsp += (256 - reinterpret_cast<uintptr_t>(wsp) % 256) % 256;")
    assert POINTER_PAD.search("base += (256 - (reinterpret_cast<uintptr_t>(base) & 255u)) & 255u;")
    assert ROUND_UP_NAME.search("static size_t align256(size_t x)") and ROUND_UP_NAME.search("pl.row_bytes = r256(M * 4);")
    header = _sources()["workspace.hpp"]
    assert "% kAlign) % kAlign" in header and "& ~(align - 1)" in header      # the one place that rounds and pads


def test_no_source_lays_a_workspace_out_by_hand():
    for name, text in _sources().items():
        if name == "workspace.hpp":
            continue
        for pattern in (ROUND_UP, POINTER_PAD, ROUND_UP_NAME):
            found = pattern.search(text)
            assert not found, (name, found.group(0))


def test_the_split_k_plan_is_defined_once():
    sources = _sources()
    assert [name for name, text in sources.items() if SPLIT_PLAN.search(text)] == ["tile_plan.hpp"]
    assert len(SPLIT_PLAN.findall(sources["tile_plan.hpp"])) == 1
    for name in ("matmul_nbits.hip", "qlinear_gemm.hip"):
        text = sources[name]
        assert '#include "tile_plan.hpp"' in text and "make_tile_plan(" in text, name
        assert not re.search(r"constexpr\s+int\s+k(BN|BK|Threads)\b", text), name      # the tile geometry too
        assert not re.search(r"\bpl\.(bm|tiles_m|tiles|steps_per_split|splits)\s*=[^=]", text), name
