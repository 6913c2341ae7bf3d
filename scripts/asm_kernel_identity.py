#!/usr/bin/env python
"""Compares, kernel by kernel, two device-assembly listings of one source file:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-inline-asm --cuda-device-only -S X.hip -o X.s

(the recipe of profiles/ops_plumbing/asm_identity.txt) from two trees.  Where a change ADDS kernels to a file, the listings differ
as wholes and the function numbers inside local labels shift; what has to hold is that every kernel of the old listing is in
the new one with the same instructions and the same kernel descriptor (registers, LDS, scratch).  A kernel's text runs from its
label to `.end_amdhsa_kernel`; local labels (.LBBn_m, .Lfunc_endn, .Ltmpn, and BBn_m in the loop comments) lose the function number n,
and runs of blanks count as one (a label's comment is padded to a column).

    python scripts/asm_kernel_identity.py [--map FILE] OLD_DIR NEW_DIR loss lovasz evaluate

prints one row per kernel of OLD_DIR/X.s and ends with the counts; exit status 1 if a kernel is missing or differs.

Where a change RENAMES kernels (two kernels folded into the instantiations of one template), --map names a file of
`old mangled name -> new mangled name` lines (blank lines and lines that start with # are skipped).  A mapped kernel is looked up under
its new name, and both texts are compared with the kernel's own name masked out; unmapped kernels compare as above."""

import os
import re
import sys

_TYPE = re.compile(r"^\s*\.type\s+(\S+),@function")
_LOCAL = re.compile(r"(\.LBB|\.Lfunc_end|\.Lfunc_begin|\.Ltmp|\bBB)\d+")


def kernels(path):
    """name -> normalised lines, for every function that has a kernel descriptor."""

    with open(path) as fp:
        lines = fp.read().split("\n")
    out, name, body = {}, None, []
    for line in lines:
        m = _TYPE.match(line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        body.append(" ".join(_LOCAL.sub(lambda k: k.group(1), line).split()))
        if line.strip() == ".end_amdhsa_kernel":
            out[name] = body
            name = None
    return out


def read_map(path):
    """old mangled name -> new mangled name."""

    renamed = {}
    with open(path) as fp:
        for line in fp:
            line = line.strip()
            if line and not line.startswith("#"):
                old, new = (part.strip() for part in line.split("->"))
                renamed[old] = new
    return renamed


def masked(body, name):
    return [line.replace(name, "<kernel>") for line in body]


def main(argv):
    argv = list(argv)
    renamed = {}
    if "--map" in argv:
        at = argv.index("--map")
        renamed = read_map(argv[at + 1])
        del argv[at:at + 2]
    old_dir, new_dir, stems = argv[1], argv[2], argv[3:]
    total = same = 0
    for stem in stems:
        old, new = kernels(os.path.join(old_dir, stem + ".s")), kernels(os.path.join(new_dir, stem + ".s"))
        for name in sorted(old):
            total += 1
            now = renamed.get(name, name)
            if now not in new:
                verdict = "missing"
            elif now == name:
                verdict = "yes" if old[name] == new[name] else "NO"
            else:
                verdict = "yes" if masked(old[name], name) == masked(new[now], now) else "NO"
            same += verdict == "yes"
            print("{:<12} {:>7}  {:<8} {}{}".format(stem + ".hip", len(old[name]), verdict, name, "" if now == name else " -> " + now))
        known = set(old) | set(renamed.values())
        print("{:<12} {} kernels before, {} after ({} new)".format(stem + ".hip", len(old), len(new), len(set(new) - known)))
    print("\n{} kernels of the old listings, {} identical, {} different or missing".format(total, same, total - same))
    return 0 if same == total else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
