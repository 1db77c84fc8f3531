#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of csrc/, kernel by kernel.

    python scripts/cmp_device_code.py OLD_BUILD_DIR NEW_BUILD_DIR [--expect-removed NAME ...]

Each build directory holds the objects of `make -C masked-diffusion-model_amd/csrc BUILD=...` (X.hip.o).  For every
object present in both, the gfx950 code object is taken out of the .hip_fatbin section, disassembled, and split at
the `<symbol>:` lines.  Three things are normalised, nothing else:
  - the `// address: encoding` comment of every instruction;
  - trailing padding at the end of a kernel (s_nop 0, `...`, s_code_end);
  - the literal of the s_add_u32 / s_addc_u32 right after an s_getpc_b64 (a pc-relative address of a global, which
    moves whenever other code moves).
Each kernel's AMDGPU metadata entry (llvm-readobj --notes: arguments, register counts, segment sizes) is compared
as text.  Prints one line per object and a summary; exits 1 if a kernel differs, a kernel was added, or the set of
removed kernels is not the one given with --expect-removed (substrings of demangled-or-mangled names).
Needs only the ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, llvm-objdump, llvm-readobj).
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
SYM = re.compile(r"^[0-9a-f]+ <(.+)>:$")
PAD = {"s_nop 0", "...", "s_code_end"}


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def code_object(obj, work):
    """X.hip.o -> (disassembly text, notes text) of its gfx950 code object."""
    base = os.path.join(work, os.path.basename(obj))
    tool("llvm-objcopy", f"--dump-section=.hip_fatbin={base}.fatbin", obj, os.devnull)
    tool("clang-offload-bundler", "--type=o", "--unbundle", f"--input={base}.fatbin", f"--targets={TARGET}", f"--output={base}.co")
    return tool("llvm-objdump", "-d", "--mcpu=gfx950", f"{base}.co"), tool("llvm-readobj", "--notes", f"{base}.co")


def kernels(dis):
    """symbol -> normalised instruction list"""
    out, cur, after_getpc = {}, None, 0
    for line in dis.splitlines():
        m = SYM.match(line.strip())
        if m:
            cur = out.setdefault(m.group(1), [])
            after_getpc = 0
            continue
        if cur is None:
            continue
        ins = line.split("//", 1)[0].strip()
        if not ins:
            continue
        if ins.startswith("s_getpc_b64"):
            after_getpc = 2
        elif after_getpc and (ins.startswith("s_add_u32") or ins.startswith("s_addc_u32")):
            ops = ins.split(",")
            ins = ",".join(ops[:-1] + [" <pcrel>"])
            after_getpc -= 1
        else:
            after_getpc = 0
        cur.append(ins)
    for v in out.values():
        while v and v[-1] in PAD:
            v.pop()
    return out


def metadata(notes):
    """kernel symbol -> its amdhsa.kernels entry (text)"""
    out, block, inside = {}, [], False

    def flush():
        if block:
            name = next((ln.split(":", 1)[1].strip() for ln in block if ln.strip().startswith(".name:")), None)
            if name:
                out[name] = "\n".join(block)

    for line in notes.splitlines():
        if line.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if inside and line and not line.startswith(" "):
            flush()
            block, inside = [], False
            continue
        if not inside:
            continue
        if line.startswith("  - "):
            flush()
            block = []
        block.append(line)
    flush()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--expect-removed", nargs="*", default=None, help="substrings naming exactly the kernels the new build drops")
    a = ap.parse_args()
    objs = sorted(f for f in os.listdir(a.old) if f.endswith(".hip.o") and os.path.exists(os.path.join(a.new, f)))
    missing = sorted(f for f in os.listdir(a.old) if f.endswith(".hip.o") and f not in objs)
    ok = not missing
    n_cmp = n_same = 0
    removed, added, differ = [], [], []
    with tempfile.TemporaryDirectory() as work:
        for f in objs:
            os.makedirs(os.path.join(work, "old"), exist_ok=True)
            os.makedirs(os.path.join(work, "new"), exist_ok=True)
            dis_o, notes_o = code_object(os.path.join(a.old, f), os.path.join(work, "old"))
            dis_n, notes_n = code_object(os.path.join(a.new, f), os.path.join(work, "new"))
            ko, kn = kernels(dis_o), kernels(dis_n)
            mo, mn = metadata(notes_o), metadata(notes_n)
            same = 0
            for k in sorted(ko.keys() & kn.keys()):
                if ko[k] == kn[k] and mo.get(k) == mn.get(k):
                    same += 1
                else:
                    why = "code" if ko[k] != kn[k] else "metadata"
                    differ.append(f"{f}: {k} ({why})")
            n_cmp += len(ko.keys() & kn.keys())
            n_same += same
            removed += [f"{f}: {k}" for k in sorted(ko.keys() - kn.keys())]
            added += [f"{f}: {k}" for k in sorted(kn.keys() - ko.keys())]
            print(f"{f}: {len(ko)} -> {len(kn)} kernels, {same} of {len(ko.keys() & kn.keys())} common ones identical")
    for k in differ:
        print("DIFFERS", k)
    for k in added:
        print("ADDED  ", k)
    for k in removed:
        print("REMOVED", k)
    for f in missing:
        print("MISSING", f, "(not in the new build)")
    print(f"summary: {n_cmp} kernels compared, {n_same} identical, {len(differ)} differ, {len(removed)} removed, {len(added)} added")
    if differ or added:
        ok = False
    if a.expect_removed is not None:
        want = set(a.expect_removed)
        hit = {s for s in want for k in removed if s in k}
        unexplained = [k for k in removed if not any(s in k for s in want)]
        if hit != want or unexplained:
            print("removed kernels do not match --expect-removed:", sorted(want - hit), unexplained)
            ok = False
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
