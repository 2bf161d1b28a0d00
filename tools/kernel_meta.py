"""The register and memory figures of every kernel in a HIP object file or code object, from the
code object's metadata note: .vgpr_count, .sgpr_count, .private_segment_fixed_size (scratch bytes
per lane) and .group_segment_fixed_size (LDS bytes).  Needs no GPU.

Usage: python tools/kernel_meta.py [--text] OBJECT [OTHER_OBJECT]
One object: a line per kernel.  Two: the kernels whose figures differ, the symbols only one of them
has, and exit status 1 if a symbol they share differs -- the check that a change to the kernels'
sources left the existing kernels' code as it was.  --text (two objects): the kernels' disassembled
text is compared as well, symbol by symbol -- the check that a refactor moved no instruction.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("AFS_LLVM_BIN", "/opt/rocm/llvm/bin")
ARCH = os.environ.get("AFS_OFFLOAD_ARCH", "gfx950")
FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernel_meta(path: str, text: dict | None = None) -> dict:
    """{kernel symbol: (vgprs, sgprs, scratch bytes, LDS bytes)} of a host object with an embedded
    code object for ARCH, or of a code object itself.  `text`, if given, receives {symbol: its
    disassembly without addresses and encodings}."""
    bundler, objcopy, readelf = (os.path.join(LLVM, t) for t in ("clang-offload-bundler", "llvm-objcopy", "llvm-readelf"))
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "device.co")
        # a host object keeps its code objects bundled in the .hip_fatbin section
        p = subprocess.run([objcopy, "--dump-section", ".hip_fatbin=" + fat, path], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        if p.returncode == 0 and os.path.exists(fat):
            subprocess.run([bundler, "--unbundle", "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}",
                            "--input=" + fat, "--output=" + co], check=True)
        else:
            co = path  # (already a code object)
        notes = subprocess.run([readelf, "--notes", co], check=True, stdout=subprocess.PIPE, text=True).stdout
        if text is not None:
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                                 check=True, stdout=subprocess.PIPE, text=True).stdout
            # "<symbol>:" opens a function; a label inside one ("<L0>:", "<symbol+0x1c>:") stays its text
            sym = None
            for line in dis.splitlines():
                m = re.match(r"^(?:[0-9a-f]+ )?<([^>+]+)>:$", line)
                if m and not re.fullmatch(r"L\d+", m.group(1)):
                    sym = m.group(1)
                    text[sym] = []
                elif sym is not None and line.strip():
                    # (this objdump still trails "// address: encoding [<branch target>]": keep the target alone)
                    ins, _, tail = line.partition("//")
                    text[sym].append(ins.strip() + " " + " ".join(re.findall(r"<[^>]+>", tail)))
    out: dict = {}
    cur: dict = {}

    def close() -> None:
        if ".name" in cur and all(f in cur for f in FIELDS):
            out[cur[".name"].strip("'\"")] = tuple(int(cur[f]) for f in FIELDS)

    # amdhsa.kernels: a list of maps, "  - .key: value" opening a kernel's and "    .key: value" going on
    # with it (its arguments' maps are indented further)
    for line in notes.splitlines():
        m = re.match(r"^  (- | {2})(\.\w+):\s*(\S+)\s*$", line)
        if line.startswith("  - "):
            close()
            cur = {}
        if m and m.group(2) in FIELDS + (".name",):
            cur[m.group(2)] = m.group(3)
    close()
    return out


def main() -> int:
    argv = [x for x in sys.argv[1:] if x != "--text"]
    with_text = len(argv) != len(sys.argv) - 1
    if len(argv) not in (1, 2) or (with_text and len(argv) != 2):
        print(__doc__)
        return 2
    ta, tb = ({}, {}) if with_text else (None, None)
    a = kernel_meta(argv[0], ta)
    if len(argv) == 1:
        for name in sorted(a):
            print(name, *a[name])
        return 0
    b = kernel_meta(argv[1], tb)
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in b:
            print("only in the first: ", name, *a[name])
        elif name not in a:
            print("only in the second:", name, *b[name])
        elif a[name] != b[name]:
            bad += 1
            print("differs:", name, a[name], "->", b[name])
    print(f"{len(set(a) & set(b))} shared kernels, {bad} differ ({' '.join(f.lstrip('.') for f in FIELDS)})")
    if with_text:  # (every function of the code objects: a device function that was not inlined counts)
        shared = sorted(set(ta) & set(tb))
        moved = [name for name in shared if ta[name] != tb[name]]
        for name in moved:
            print("text differs:", name, len(ta[name]), "->", len(tb[name]), "lines")
        print(f"{len(shared) - len(moved)} of {len(shared)} shared functions disassemble to the same text")
        bad += len(moved) + (not shared)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
