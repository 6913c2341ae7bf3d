#!/usr/bin/env python3
"""Instruction counts per basic block of one kernel in a gfx950 assembly listing (hipcc -S --cuda-device-only), by class.

    python scripts/wino33_icount.py conv_wino33_f32.s conv_wino33_f32_kernelILi4ELi2ELi1E [--loops | --path L1,L2,...]

Prints one row per basic block in layout order (a block ends at a label or behind a branch; "<label>+k" is the k-th piece behind
<label>): name, instructions by class (mfma, valu, salu, lds, vmem, wait = s_waitcnt / s_nop /
s_barrier, branch), how it ends and where it can go.  With --path: the sum over the named blocks (the blocks a wave walks for one chunk
or one item, read off the branch structure; "entry" names the block before the first label).  No GPU involved: these are the static
counts behind profiles/wino33_items/README.md."""
import argparse
import re
import sys

CLASSES = ("mfma", "valu", "salu", "lds", "vmem", "wait", "branch")
DEPTH = {}  # label -> loop depth of the block (0: outside every loop)


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op in ("s_waitcnt", "s_nop", "s_barrier") or op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    return None


def blocks_of(path, kernel):
    """[(label, {class: n}, [branch targets], falls_through)] of the first kernel whose symbol contains `kernel`."""
    out, cur, inside = [], None, False
    with open(path) as fp:
        for line in fp:
            s = line.split(";")[0].rstrip()
            if not inside:
                m = re.match(r"^(\S+):", s)
                if m and kernel in m.group(1) and not m.group(1).startswith("."):
                    inside = True
                    cur = ["entry", dict.fromkeys(CLASSES, 0), [], True]
                continue
            if s.strip().startswith(".Lfunc_end") or s.strip().startswith(".section"):
                break
            m = re.match(r"^(\.LBB\S+):", s)
            if m:
                out.append(tuple(cur))
                cur = [m.group(1), dict.fromkeys(CLASSES, 0), [], True]
                d = re.search(r"Depth=(\d+)", line)  # (hipcc's loop annotation: "in Loop: Header=... Depth=1", "Inner Loop Header: Depth=2")
                # (an inner loop's header is printed as "Parent Loop BBx Depth=1" with its own depth on the next line)
                DEPTH[m.group(1)] = (int(d.group(1)) + ("Parent Loop" in line)) if d else 0
                continue
            for piece in s.split("\\n\\t"):  # (inline asm with several instructions per statement is printed on separate lines already)
                tok = piece.split()
                if not tok or tok[0].startswith("."):
                    continue
                cls = classify(tok[0])
                if cls is None:
                    continue
                cur[1][cls] += 1
                if cls == "branch":  # a branch ends the block: what follows it up to the next label is "<label>+k"
                    if len(tok) > 1 and tok[1].startswith(".LBB"):
                        cur[2].append(tok[1])
                    cur[3] = tok[0].startswith("s_cbranch")
                    out.append(tuple(cur))
                    base, _, k = cur[0].partition("+")
                    cur = ["{}+{}".format(base, int(k or 0) + 1), dict.fromkeys(CLASSES, 0), [], True]
    if cur:
        out.append(tuple(cur))
    return [blk for blk in out if sum(blk[1].values())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("kernel", help="substring of the kernel's (mangled) symbol")
    ap.add_argument("--path", help="comma-separated block labels to sum (a label may repeat)")
    ap.add_argument("--loops", action="store_true", help="sums per loop level instead of per block")
    a = ap.parse_args()
    blocks = blocks_of(a.asm, a.kernel)
    if not blocks:
        sys.exit("no kernel matching " + a.kernel)
    if a.loops:
        # the kernel's two loops: depth 1 = the block's items, depth 2 = an item's chunks from the second one on (hipcc peels the first
        # chunk, which carries the kc == 0 work, into the item loop).  Sums over ALL blocks of a depth: an upper bound of any one walk
        # (mutually exclusive branches are both counted).
        seen_loop, tot = False, {k: dict.fromkeys(CLASSES, 0) for k in ("before the loops", "item loop, outside the chunk loop", "chunk loop", "behind the loops")}
        for lab, cnt, _, _ in blocks:
            d = DEPTH.get(lab.partition("+")[0], 0)
            seen_loop = seen_loop or d > 0
            key = "chunk loop" if d >= 2 else "item loop, outside the chunk loop" if d == 1 else "behind the loops" if seen_loop else "before the loops"
            for c in CLASSES:
                tot[key][c] += cnt[c]
        print("{:<36}".format("region") + "".join("{:>7}".format(c) for c in CLASSES) + "  non-mfma")
        for key, t in tot.items():
            print("{:<36}".format(key) + "".join("{:>7}".format(t[c]) for c in CLASSES) + "{:>10}".format(sum(t.values()) - t["mfma"]))
        return
    if a.path:
        by = {b[0]: b[1] for b in blocks}
        tot = dict.fromkeys(CLASSES, 0)
        for lab in a.path.split(","):
            for c in CLASSES:
                tot[c] += by[lab][c]
        print(" ".join("{}={}".format(c, tot[c]) for c in CLASSES), "non-mfma={}".format(sum(tot.values()) - tot["mfma"]))
        return
    print("{:<14}".format("block") + "".join("{:>7}".format(c) for c in CLASSES) + "  -> targets")
    for lab, cnt, tg, ft in blocks:
        print("{:<14}".format(lab) + "".join("{:>7}".format(cnt[c]) for c in CLASSES) + "  -> " + ", ".join(tg) + (" | next" if ft else ""))


if __name__ == "__main__":
    main()
