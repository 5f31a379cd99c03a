#!/usr/bin/env python
"""Print one digest of the gfx950 assembly of every source of libmuon_amd.so: `source  sha256  line-count`.

Two checkouts whose listings are equal compile to the same device code; a refactor that only moves inlined helpers
is proved by that.  The lines that carry the `__hip_cuid_<hash>` symbol are dropped first: the hash is of the source
text.  This only hashes; it looks for nothing in the assembly.

Usage: python scripts/isa_digest.py [--root OTHER_CHECKOUT]
(the checkout at --root is compiled by its own muon_amd/csrc/build.py, which must have device_asm)
"""
import argparse
import hashlib
import importlib.util
import os
import tempfile
from concurrent.futures import ThreadPoolExecutor


def load_build(root):
    path = os.path.join(os.path.abspath(root), "muon_amd", "csrc", "build.py")
    spec = importlib.util.spec_from_file_location("isa_digest_build", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def digest(build, source, tmp):
    out = build.device_asm(source, os.path.join(tmp, source + ".s"))
    with open(out) as f:
        lines = [l for l in f if "__hip_cuid_" not in l]
    return hashlib.sha256("".join(lines).encode()).hexdigest(), len(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    build = load_build(args.root)
    print("# " + build._compiler_id())
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(8) as pool:
        for source, (sha, n) in zip(build.SOURCES, pool.map(lambda s: digest(build, s, tmp), build.SOURCES)):
            print(f"{source:<20} {sha}  {n}", flush=True)


if __name__ == "__main__":
    main()
