#!/usr/bin/env python3
"""Compare the gfx950 instruction streams of every kernel in two sets of object files (a build before and after a change).

usage: tools/isa_diff.py BEFORE_DIR AFTER_DIR [file.o ...]
       (default: every *.o in BEFORE_DIR; e.g. BEFORE_DIR = a copy of mfcc-rust_amd/lib/*.o from the parent commit's build)

Each .o's device code object is taken from its .hip_fatbin section, unbundled and disassembled (llvm-objcopy,
clang-offload-bundler, llvm-objdump).  A kernel is keyed by its demangled name, in which an empty template pack does not appear:
an instantiation whose template gained an empty trailing pack is still paired with its old self.  Addresses and padding are
removed and branch targets rewritten relative to the kernel's start.  Prints, per file, the kernels that are identical, changed,
only before and only after; exits 1 if a kernel of BEFORE is missing or changed.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def kernels(obj: str) -> dict:
    with tempfile.TemporaryDirectory() as td:
        fb, co = os.path.join(td, "fatbin"), os.path.join(td, "dev.co")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj, os.path.join(td, "rest.o")], check=True,
                       capture_output=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", f"--targets={TARGET}", f"--input={fb}", f"--output={co}",
                        "--unbundle"], check=True)
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--demangle", co], check=True,
                             capture_output=True, text=True).stdout
    out, name, base, body = {}, None, 0, []
    for line in dis.splitlines():
        m = re.match(r"^([0-9a-f]+) <(.*)>:$", line)
        if m:
            if name is not None:
                out[name] = body
            base, body = int(m.group(1), 16), []
            name = re.sub(r", >|<>", lambda t: ">" if t.group(0) == ", >" else "", m.group(2))
            continue
        if name is None or not line.strip():
            continue
        ins = re.sub(r"\s*//\s*[0-9A-Fa-f]+:.*$", "", line).strip()  # the address comment
        # branch targets: absolute address -> offset from the kernel's start
        ins = re.sub(r"<([^<>]*)\+0x([0-9a-f]+)>", lambda t: f"<+{int(t.group(2), 16)}>", ins)
        ins = re.sub(r"\b0x([0-9a-f]+) <\+", "<+", ins)
        if ins.startswith("s_code_end") or ins == "...":  # (padding between kernels: depends on the layout only)
            continue
        body.append(ins)
    if name is not None:
        out[name] = body
    return out


def main() -> int:
    before, after = sys.argv[1], sys.argv[2]
    files = sys.argv[3:] or sorted(f for f in os.listdir(before) if f.endswith(".o"))
    bad = 0
    for f in files:
        try:
            kb, ka = kernels(os.path.join(before, f)), kernels(os.path.join(after, f))
        except subprocess.CalledProcessError:
            print(f"{f}: no gfx950 device code")
            continue
        same = [k for k in kb if k in ka and kb[k] == ka[k]]
        changed = [k for k in kb if k in ka and kb[k] != ka[k]]
        gone = [k for k in kb if k not in ka]
        new = [k for k in ka if k not in kb]
        print(f"{f}: {len(same)} identical, {len(changed)} changed, {len(gone)} only before, {len(new)} new")
        for k in changed:
            print(f"  CHANGED  {k}")
        for k in gone:
            print(f"  MISSING  {k}")
        for k in new:
            print(f"  new      {k}")
        bad += len(changed) + len(gone)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
