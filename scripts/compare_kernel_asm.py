#!/usr/bin/env python3
"""Do two checkouts compile the same gfx950 kernels?  Text comparison of the device assembly, kernel by kernel.

    python scripts/compare_kernel_asm.py PARENT_CHECKOUT CHANGE_CHECKOUT awq.hip rtn_mse.hip ... [--keep DIR]

Each source of onnx_quantize_amd/csrc is compiled in both checkouts with that checkout's own `_build.flags_for(src)` plus
`-S --cuda-device-only`.  A kernel is the text from its label to `.end_amdhsa_kernel`: its instructions and its `.amdhsa_`
descriptor.  Kernels are keyed by their demangled name, because instantiation order may move them inside the file and a renamed
template argument changes the mangled name (and the numbering of its substitutions).  RENAMES maps the parent's names onto the
change's; a parent kernel that still has no partner is tried once more with a leading `bool` template argument read as the
element type it selected (false: ElemF16, true: ElemBF16).  Inside a kernel's text its own mangled name and the per-function
counters of local labels are masked and the assembler's comments dropped (loop notes that repeat those counters), nothing else:
every instruction, operand, label position and descriptor line is compared.

Prints one line per source -- kernel count, identical yes / no -- and the names that differ; exit status 1 if anything does.
No GPU is needed.  `--keep DIR` leaves the .s files there (DIR/parent, DIR/change).
"""
from __future__ import annotations

import argparse
import concurrent.futures
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

RENAMES = [(re.compile(r"\boq::(Awq|Mse|Hqq)F32\b"), "oq::ElemF32")]
BOOL_ELEM = {"false": "oq::ElemF16", "true": "oq::ElemBF16"}


def _build_module(checkout: str):
    path = os.path.join(checkout, "onnx_quantize_amd", "_build.py")
    spec = importlib.util.spec_from_file_location("_oq_build_" + str(abs(hash(checkout))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_asm(checkout: str, source: str, out_dir: str) -> str:
    b = _build_module(checkout)
    src = os.path.join(checkout, "onnx_quantize_amd", "csrc", source)
    out = os.path.join(out_dir, source[:-4] + ".s")
    r = subprocess.run([b.hipcc(), *b.flags_for(src), "-S", "--cuda-device-only", "-o", out, src], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr[-4000:]}")
    return out


def demangle(names: list[str]) -> list[str]:
    exe = shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    if not os.path.exists(exe):
        exe = shutil.which("c++filt")
    if not exe or not names:
        return list(names)
    r = subprocess.run([exe], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
    return r.stdout.splitlines()


def kernels(asm_path: str) -> dict[str, str]:
    """demangled kernel name -> masked text of the kernel (label .. .end_amdhsa_kernel)"""
    with open(asm_path) as f:
        text = f.read()
    mangled = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\s*$", text, re.M)
    out = {}
    for name, pretty in zip(mangled, demangle(mangled)):
        start = text.index(f"\n{name}:") + 1
        end = text.index(".end_amdhsa_kernel", start)
        body = text[start:end].replace(name, "<kernel>")
        body = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1", body)      # per-function counters of local labels
        body = re.sub(r"[ \t]*;.*$", "", body, flags=re.M)                       # comments carry the same counters (loop notes)
        body = "\n".join(line for line in body.splitlines() if line.strip())
        assert pretty not in out, pretty
        out[pretty] = body
    return out


def _renamed(name: str) -> str:
    for pat, repl in RENAMES:
        name = pat.sub(repl, name)
    return name


def _bool_as_elem(name: str) -> str:
    return re.sub(r"<(false|true)\b", lambda m: "<" + BOOL_ELEM[m.group(1)], name, count=1)


def compare(parent: dict[str, str], change: dict[str, str]) -> tuple[list[str], list[str], list[str]]:
    """(kernels whose text differs, parent kernels without a partner, change kernels without a partner)"""
    left = dict(change)
    differ, lost = [], []
    for name, body in parent.items():
        key = _renamed(name)
        if key not in left:
            key = _bool_as_elem(key)
        if key not in left:
            lost.append(name)
            continue
        if left.pop(key) != body:
            differ.append(key)
    return differ, lost, sorted(left)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("change")
    ap.add_argument("sources", nargs="+", help="file names under onnx_quantize_amd/csrc, e.g. awq.hip")
    ap.add_argument("--keep", metavar="DIR", help="keep the assembly files here")
    a = ap.parse_args()
    work = a.keep or tempfile.mkdtemp(prefix="oq_asm_")
    dirs = {side: os.path.join(work, side) for side in ("parent", "change")}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
    jobs = [(side, checkout, s) for side, checkout in (("parent", a.parent), ("change", a.change)) for s in a.sources]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
        paths = list(ex.map(lambda j: compile_asm(os.path.abspath(j[1]), j[2], dirs[j[0]]), jobs))
    asm = {(side, s): p for (side, _, s), p in zip(jobs, paths)}
    bad = False
    for s in a.sources:
        p, c = kernels(asm[("parent", s)]), kernels(asm[("change", s)])
        differ, lost, new = compare(p, c)
        same = not (differ or lost or new)
        bad = bad or not same
        print(f"{s}: {len(p)} kernels at the parent, {len(c)} at the change, identical: {'yes' if same else 'NO'}")
        for label, names in (("text differs", differ), ("only at the parent", lost), ("only at the change", new)):
            for n in names:
                print(f"    {label}: {n}")
    if not a.keep:
        shutil.rmtree(work, ignore_errors=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
