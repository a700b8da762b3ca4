#!/usr/bin/env python3
"""Compare the gfx950 device code of two object files, symbol by symbol.

usage: tools/isa_diff.py A.o B.o [--arch gfx950] [--expect-gone REGEX] [--show N]

Each object (a hipcc fat object, or a bare device ELF) has its device ELF unbundled with
clang-offload-bundler and disassembled with `llvm-objdump -d --no-show-raw-insn`; addresses are
stripped, so a function that merely moved compares equal.  Per kernel, the metadata of
`llvm-readelf --notes` (VGPR/SGPR counts, spills, scratch, LDS, kernarg size, workgroup size) is
compared too.  Every symbol that differs, or exists on one side only, is printed; the exit status
is 0 only when there is none.  --expect-gone names symbols (demangled or not, a regex searched in
the name) that B is meant to have dropped: they are listed but do not fail the comparison.

A refactor of a kernel file is checked with it before it goes near a GPU: identical device code
means identical device behaviour and speed.
"""
from __future__ import annotations

import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM_DIRS = [os.environ.get("LLVM_BIN", ""), "/opt/rocm/lib/llvm/bin", "/opt/rocm/llvm/bin"]
META_KEYS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
             ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size",
             ".max_flat_workgroup_size", ".wavefront_size", ".uses_dynamic_stack")


def tool(name: str) -> str:
    for d in LLVM_DIRS:
        if d and os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    p = shutil.which(name)
    if not p:
        sys.exit(f"isa_diff: {name} not found (set LLVM_BIN)")
    return p


def run(*cmd: str) -> str:
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def device_elf(obj: str, arch: str, tmp: str, tag: str) -> str:
    """The device ELF of obj: a host object carries the bundle in its .hip_fatbin section; a
    bundle is unbundled as it is; a bare device ELF (--cuda-device-only) is returned unchanged."""
    with open(obj, "rb") as f:
        data = f.read()
    bundle = obj
    if data[:4] == b"\x7fELF":
        if b"__CLANG_OFFLOAD_BUNDLE__" not in data:
            return obj
        bundle = os.path.join(tmp, f"{tag}.fatbin")
        run(tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={bundle}", obj, os.devnull)
    targets = run(tool("clang-offload-bundler"), "--list", "--type=o", f"--input={bundle}").split()
    want = [t for t in targets if t.startswith("hip") and re.search(rf"-{arch}(:|$)", t)]
    if len(want) != 1:
        sys.exit(f"isa_diff: {obj}: no single {arch} target among {targets}")
    out = os.path.join(tmp, f"{tag}.elf")
    run(tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--input={bundle}", f"--targets={want[0]}",
        f"--output={out}")
    return out


SYM = re.compile(r"^[0-9a-f]+ <(.+)>:$")
# an instruction line: "\ts_load_dword s3, s[0:1], 0x9c    // 0000000F9100: C00200C0 0000009C"; the
# trailing column (address and encoding) goes, so a function that merely moved compares equal
INSN = re.compile(r"^\s+(?:[0-9a-f]+:\s+)?(\S.*?)\s*(?://\s*([0-9A-Fa-f]+):.*)?$")
# A linked code object addresses its globals relative to the program counter:
#   s_getpc_b64 s[0:1]; s_add_u32 s0, s0, <target - pc>; s_addc_u32 s1, s1, <high half>
# The distance changes whenever any code between the two changes size, so the literal is replaced
# by what it points at (section or symbol + offset).
GETPC = re.compile(r"^s_getpc_b64 s\[(\d+):(\d+)\]$")
PCADD = re.compile(r"^(s_add_u32 s(\d+), s(\d+), )(0x[0-9a-f]+|-?\d+)$")
PCADDC = re.compile(r"^(s_addc_u32 s(\d+), s(\d+), )(0x[0-9a-f]+|-?\d+)$")


def places(elf: str) -> list[tuple[int, int, str]]:
    """(address, size, name) of the allocated sections and the sized symbols, symbols last."""
    out = []
    for line in run(tool("llvm-readelf"), "-S", "-W", elf).splitlines():
        m = re.match(r"^\s*\[\s*\d+\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+[0-9a-f]+\s+([0-9a-f]+)\s", line)
        if m and int(m.group(2), 16):
            out.append((int(m.group(2), 16), int(m.group(3), 16), m.group(1)))
    for line in run(tool("llvm-readelf"), "-s", "-W", elf).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] in ("OBJECT", "FUNC") and f[2].isdigit() and int(f[2]):
            out.append((int(f[1], 16), int(f[2]), f[7]))
    return out


def place_of(addr: int, where: list[tuple[int, int, str]]) -> str:
    hit = "?"
    for a, n, name in where:   # the last match wins: a symbol over its section
        if a <= addr < a + n:
            hit = f"{name}+{addr - a:#x}"
    return hit


def functions(elf: str) -> dict[str, list[str]]:
    """symbol -> its instructions, addresses stripped (branch targets kept symbol-relative)."""
    out: dict[str, list[str]] = {}
    where = places(elf)
    cur = None
    pc_reg, pc = -1, 0      # after s_getpc_b64: its low register, the address it yields
    for line in run(tool("llvm-objdump"), "-d", "--no-show-raw-insn", elf).splitlines():
        m = SYM.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
            pc_reg = -1
            continue
        mi = INSN.match(line)
        if cur is None or not mi:
            continue
        insn = mi.group(1)
        g, a, c = GETPC.match(insn), PCADD.match(insn), PCADDC.match(insn)
        if g and mi.group(2):
            pc_reg, pc = int(g.group(1)), int(mi.group(2), 16) + 4
        elif a and pc_reg >= 0 and int(a.group(2)) == int(a.group(3)) == pc_reg:
            lit = int(a.group(4), 0) & 0xffffffff
            insn = a.group(1) + "<" + place_of(pc + lit - (1 << 32 if lit >> 31 else 0), where) + ">"
        elif c and pc_reg >= 0 and int(c.group(2)) == int(c.group(3)) == pc_reg + 1:
            insn = c.group(1) + "<hi>"
            pc_reg = -1
        cur.append(insn)
    return out


def kernel_meta(elf: str) -> dict[str, dict[str, str]]:
    """kernel name -> the code-object metadata fields that describe its resources."""
    # the note is YAML: "amdhsa.kernels:" then one "  - .field: value" item per kernel, its other
    # fields at four spaces, its arguments nested deeper
    out: dict[str, dict[str, str]] = {}
    fields: dict[str, str] = {}
    in_kernels = False

    def flush() -> None:
        if fields.get(".name"):
            out[fields[".name"]] = {k: fields.get(k, "") for k in META_KEYS}
        fields.clear()

    for line in run(tool("llvm-readelf"), "--notes", elf).splitlines():
        if line.startswith("amdhsa.kernels:"):
            in_kernels = True
            continue
        if in_kernels and re.match(r"^\S", line):   # the next top-level key
            in_kernels = False
        if not in_kernels:
            continue
        m = re.match(r"^  (- |  )(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) == "- ":
            flush()
        fields[m.group(2)] = m.group(3).strip("'\"")
    flush()
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--expect-gone", default=None, metavar="REGEX")
    ap.add_argument("--show", type=int, default=0, metavar="N",
                    help="print the differing instructions among the first N from the first difference")
    args = ap.parse_args()
    gone_ok = re.compile(args.expect_gone) if args.expect_gone else None
    with tempfile.TemporaryDirectory() as tmp:
        ea, eb = device_elf(args.a, args.arch, tmp, "a"), device_elf(args.b, args.arch, tmp, "b")
        fa, fb = functions(ea), functions(eb)
        ma, mb = kernel_meta(ea), kernel_meta(eb)
    bad = 0
    for name in sorted(set(fa) | set(fb)):
        if name not in fb:
            ok = gone_ok is not None and gone_ok.search(name)
            print(f"{'gone (expected)' if ok else 'ONLY IN A'}: {name} ({len(fa[name])} instructions)")
            bad += 0 if ok else 1
        elif name not in fa:
            print(f"ONLY IN B: {name} ({len(fb[name])} instructions)")
            bad += 1
        elif fa[name] != fb[name]:
            first = next((i for i, (x, y) in enumerate(zip(fa[name], fb[name])) if x != y),
                         min(len(fa[name]), len(fb[name])))
            print(f"DIFFERS: {name}: {len(fa[name])} -> {len(fb[name])} instructions, first at #{first}")
            for i in range(first, min(first + args.show, len(fa[name]), len(fb[name]))):
                if fa[name][i] != fb[name][i]:
                    print(f"    #{i}: {fa[name][i]}  |  {fb[name][i]}")
            bad += 1
    for name in sorted(set(ma) | set(mb)):
        if name in ma and name in mb and ma[name] != mb[name]:
            d = ", ".join(f"{k} {ma[name][k]} -> {mb[name][k]}" for k in META_KEYS if ma[name][k] != mb[name][k])
            print(f"METADATA DIFFERS: {name}: {d}")
            bad += 1
        elif (name in ma) != (name in mb) and not (name in ma and gone_ok and gone_ok.search(name)):
            print(f"METADATA ONLY IN {'A' if name in ma else 'B'}: {name}")
            bad += 1
    print(f"{len(fa)} functions / {len(ma)} kernels in A, {len(fb)} / {len(mb)} in B: "
          f"{'identical' if not bad else str(bad) + ' differences'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
