#!/usr/bin/env python3
"""Device-code comparison of two builds, kernel by kernel: the check for a refactor that moves kernel source between
files or namespaces and must not change what the compiler emits.  No GPU needed.

Each side is the gfx950 assembly of one or more units, compiled with the flags of build.py:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics -I <csrc> --cuda-device-only -S unit.hip -o unit.s
    python tools/kernel_asm_diff.py old/dwconv.s -- new/dw_fwd.s new/dw_bwd_s1.s new/dw_bwd_s2.s

A kernel is keyed by its demangled name and template arguments with namespace qualifiers stripped, so a kernel that
moved to another unit, or whose parameter structs moved to another namespace, still pairs with itself.  Compared per
kernel: the instructions, the .amdhsa descriptor block, the resource symbols (.set <kernel>.num_vgpr, ...) and the
code-object metadata entry (registers, spills, scratch, LDS, argument layout), with comments stripped, the kernel's
own symbol replaced and local labels renumbered in order of appearance.  Exit status 1 if the sets of kernels differ
or any kernel differs.
"""
import re
import subprocess
import sys

QUAL = re.compile(r"(\(anonymous namespace\)|\b[A-Za-z_]\w*)::")
LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def strip_qualifiers(name: str) -> str:
    return QUAL.sub("", name)


def normalise(lines, sym):
    labels = {}
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip().replace(sym, "KERNEL")
        if ln.strip():
            out.append(LABEL.sub(lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), ln))
    return out


def kernels(path):
    """{mangled symbol: normalised text} of every kernel in one assembly file"""
    lines = open(path).read().split("\n")
    syms = [m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m]
    meta = {}
    if "\t.amdgpu_metadata" in lines:
        block = lines[lines.index("\t.amdgpu_metadata"):lines.index("\t.end_amdgpu_metadata")]
        for entry in "\n".join(block).split("\n  - ")[1:]:
            entry = re.split(r"\n(?=\S)", entry)[0]          # the last entry ends where the next top-level key begins
            name = re.search(r"\.name:\s+(\S+)", entry)       # (amdhsa.version's items have none)
            if name:
                meta[name.group(1)] = entry.split("\n")
    out = {}
    for sym in syms:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(sym + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith("\t.size\t" + sym + ","))
        sets = [ln for ln in lines[end:end + 40] if ln.startswith("\t.set " + sym + ".")]
        out[sym] = normalise(lines[start:end + 1] + sets + meta.get(sym, ["<no metadata entry>"]), sym)
    return out


def side(paths):
    """{qualifier-free demangled name: (file, normalised text)} over the files of one side"""
    found = {}
    for p in paths:
        ks = kernels(p)
        names = subprocess.run(["c++filt"], input="\n".join(ks), capture_output=True, text=True,
                               check=True).stdout.splitlines()
        for sym, name in zip(ks, names):
            key = strip_qualifiers(name)
            if key in found:
                raise SystemExit(f"{key}: defined in {found[key][0]} and in {p}")
            found[key] = (p, ks[sym])
    return found


def main():
    if "--" not in sys.argv[2:-1]:
        raise SystemExit(__doc__)
    cut = sys.argv.index("--")
    a, b = side(sys.argv[1:cut]), side(sys.argv[cut + 1:])
    for k in sorted(set(a) - set(b)):
        print(f"only in the first:  {k}")
    for k in sorted(set(b) - set(a)):
        print(f"only in the second: {k}")
    differ = [k for k in sorted(set(a) & set(b)) if a[k][1] != b[k][1]]
    for k in differ:
        n = next((i for i, (x, y) in enumerate(zip(a[k][1], b[k][1])) if x != y), min(len(a[k][1]), len(b[k][1])))
        print(f"differs: {k}\n  {a[k][0]} ({len(a[k][1])} lines) / {b[k][0]} ({len(b[k][1])} lines), first at line {n}:")
        print(f"    {a[k][1][n] if n < len(a[k][1]) else '<end>'}\n    {b[k][1][n] if n < len(b[k][1]) else '<end>'}")
    same = len(set(a) & set(b)) - len(differ)
    print(f"{len(a)} kernels in the first, {len(b)} in the second, {len(set(a) & set(b))} in both: {same} identical, "
          f"{len(differ)} differ")
    return 0 if set(a) == set(b) and not differ else 1


if __name__ == "__main__":
    sys.exit(main())
