#!/usr/bin/env python
"""Compare the gfx950 assembly of two checkouts kernel by kernel: `source  parent  branch  identical  different  only`.

For every name in the branch's build.SOURCES both trees are compiled by their own muon_amd/csrc/build.py
(`device_asm`: the flags the library is built with), each dump is cut into kernels - from the kernel's label to its
`.end_amdhsa_kernel`, the `.amdhsa_*` directives included - and comments (`; ...`, whole lines and line ends) and the
`__hip_cuid_<hash>` lines (a hash of the source text) are dropped.  Local labels carry the kernel's position in its
file (`.LBB<n>_`, `.Lfunc_end<n>`): the position is taken out, so a kernel that merely moved compares equal.  A refactor
of host code leaves every kernel identical and none in one tree only; the order of the kernels inside a file may differ
and is reported.  Exit status 1 if anything differs.

Usage: python scripts/kernel_asm_diff.py PARENT_CHECKOUT BRANCH_CHECKOUT [source.hip ...]
"""
import os
import re
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_digest import load_build  # noqa: E402

_KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
_POSITION = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+")


def kernels(path):
    """{kernel symbol: its lines} of one assembly dump, in the file's order."""
    with open(path) as f:
        lines = [_POSITION.sub(r".\1", l.split(";")[0].rstrip()) for l in f]
    lines = [l for l in lines if l.strip() and "__hip_cuid_" not in l]
    names = [m.group(1) for m in map(_KERNEL.match, lines) if m]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        out[name] = lines[start:end + 1]
    return out


def compare(source, parent, branch, tmp):
    a = kernels(parent.device_asm(source, os.path.join(tmp, "parent_" + source + ".s")))
    b = kernels(branch.device_asm(source, os.path.join(tmp, "branch_" + source + ".s")))
    both = [k for k in a if k in b]
    return {"parent": len(a), "branch": len(b), "identical": sum(a[k] == b[k] for k in both),
            "different": [k for k in both if a[k] != b[k]], "only": sorted(set(a) ^ set(b)),
            "reordered": both != [k for k in b if k in a]}


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    parent, branch = load_build(sys.argv[1]), load_build(sys.argv[2])
    sources = sys.argv[3:] or branch.SOURCES
    bad = False
    print("| file | kernels, parent | kernels, branch | identical | different | only in one tree | order |")
    print("|---|---:|---:|---:|---:|---:|---|")
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(4) as pool:
        for source, r in zip(sources, pool.map(lambda s: compare(s, parent, branch, tmp), sources)):
            print(f"| `{source}` | {r['parent']} | {r['branch']} | {r['identical']} | {len(r['different'])} | "
                  f"{len(r['only'])} | {'differs' if r['reordered'] else 'same'} |", flush=True)
            for k in r["different"]:
                print(f"  different: {k}")
            for k in r["only"]:
                print(f"  only in one tree: {k}")
            bad = bad or bool(r["different"] or r["only"])
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
