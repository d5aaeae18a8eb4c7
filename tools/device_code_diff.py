#!/usr/bin/env python3
"""Which device functions did a change move?  Builds the gfx950 code object of two trees and compares it symbol by symbol.

    tools/device_code_diff.py BEFORE AFTER [--must-match REGEX]...

BEFORE and AFTER are source trees, git revisions of the repository this file lies in (checked out to a temporary directory), or code
objects this recipe built earlier.  A tree is compiled with its own build.HIPCC_FLAGS, device side only: no GPU is needed.  Per function
symbol of .text: whether the bytes, taken through the symbol table's offset and size, are identical; the size on either side; for
kernels, from the code object's metadata note, VGPRs, SGPRs, scratch and LDS bytes and the waves per SIMD those allow.  Names are the
mangled ones, and REGEX is searched in them.  Exit status 1 when a symbol that a --must-match names differs or exists on one side only,
or when a --must-match names nothing.  A function that calls another one holds the distance between the two: it keeps its bytes only
while the functions between them keep their order and sizes.
"""
from __future__ import annotations

import argparse
import hashlib
import importlib.util
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_code_object(tree: str, out: str) -> str:
    spec = importlib.util.spec_from_file_location("_lw_build", os.path.join(tree, "open_ludwig_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    flags = [f for f in build.HIPCC_FLAGS if f != "-shared"]
    cmd = [build.hipcc_path(), *flags, "--cuda-device-only", "--no-gpu-bundle-output", "-c", *build.SOURCES, "-o", out]
    subprocess.run(cmd, cwd=build.CSRC, check=True)
    return out


def functions(path: str):
    """{name: bytes} of the FUNC symbols, and the .text section"""
    with open(path, "rb") as fh:
        elf = fh.read()
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", elf, 0x3A)
    sh = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]   # name type flags addr off size link ..
    symtab = next(s for s in sh if s[1] == 2)
    strtab = sh[symtab[6]]
    out = {}
    for o in range(symtab[4], symtab[4] + symtab[5], 24):
        name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, o)
        if info & 0xF != 2 or not 0 < shndx < shnum:        # STT_FUNC, defined
            continue
        end = elf.index(b"\0", strtab[4] + name)
        start = value - sh[shndx][3] + sh[shndx][4]
        out[elf[strtab[4] + name:end].decode()] = elf[start:start + size]
    text = next(s for s in sh if s[1] == 1 and s[2] & 4)     # PROGBITS, executable
    return out, elf[text[4]:text[4] + text[5]]


def kernel_resources(path: str):
    """{kernel name: metadata dict} from the NT_AMDGPU_METADATA note, as llvm-readelf prints it"""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")))
    readelf = shutil.which("llvm-readelf") or os.path.join(rocm, "llvm", "bin", "llvm-readelf")
    text = subprocess.run([readelf, "--notes", path], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^  (- |  )\.(\w+):\s+(.*)$", line)    # kernel-level keys only: the arguments' are indented deeper
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if cur is not None:
            cur[m.group(2)] = m.group(3).strip("'\"")
            if m.group(2) == "name":
                kernels[cur["name"]] = cur
    return kernels


def resources(meta) -> str:
    if meta is None:
        return "(no kernel)"
    vgpr, lds = int(meta["vgpr_count"]), int(meta["group_segment_fixed_size"])
    waves = min(8, 512 // max(8, -(-vgpr // 8) * 8))         # 512 registers per lane, granule 8
    if lds:                                                  # 160 KiB per CU, four SIMDs
        waves = min(waves, (163840 // lds) * -(-int(meta["max_flat_workgroup_size"]) // 64) // 4)
    return f"v{vgpr} s{meta['sgpr_count']} scratch{meta['private_segment_fixed_size']} lds{lds} waves{waves}"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--must-match", action="append", default=[], metavar="REGEX")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        sides = []
        for i, where in enumerate((args.before, args.after)):
            tree = where
            if not os.path.exists(where):
                tree = os.path.join(tmp, f"tree{i}")
                os.mkdir(tree)
                archive = subprocess.run(["git", "-C", REPO, "archive", where], check=True, capture_output=True).stdout
                subprocess.run(["tar", "-x", "-C", tree], input=archive, check=True)
            obj = where if os.path.isfile(where) else build_code_object(tree, os.path.join(tmp, f"device{i}.co"))
            funcs, text = functions(obj)
            sides.append((funcs, kernel_resources(obj)))
            print(f"{where}: .text {len(text)} bytes, sha256 {hashlib.sha256(text).hexdigest()}, {len(funcs)} functions")
    (fa, ka), (fb, kb) = sides
    differing = []
    for name in sorted(set(fa) | set(fb)):
        a, b = fa.get(name), fb.get(name)
        same = a is not None and a == b
        if not same:
            differing.append(name)
        size = lambda f: "-" if f is None else str(len(f))
        ra, rb = resources(ka.get(name)), resources(kb.get(name))
        print(f"{'identical' if same else 'DIFFERS  '} {size(a):>6} {size(b):>6}  {ra if ra == rb else ra + ' -> ' + rb}  {name}")
    failed = False
    for rx in args.must_match:
        named = [n for n in set(fa) | set(fb) if re.search(rx, n)]
        bad = sorted(n for n in named if n in differing)
        print(f"--must-match {rx}: {len(named)} symbols, {len(bad)} differ" + "".join("\n    " + n for n in bad))
        failed |= bool(bad) or not named
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
