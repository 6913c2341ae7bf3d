#!/usr/bin/env python
"""A/B of the loss kernels across two builds of the library, with the protocol of profiles/ignore_label/README.md.

    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python scripts/loss_variants_ab.py run --classes 2
    python scripts/loss_variants_ab.py table parent_a=DIR new_a=DIR parent_b=DIR new_b=DIR

`run` launches, 3 + 20 times at N = 32, 512 x 512, the entry points whose kernels are to be compared: CrossEntropy and Focal with a
pixel-weight plane (forward + backward), Lovasz and Lovasz-Softmax (per image, with the gradient) plain and with 30 % of the
pixels ignored.  It goes through robosat_amd.ops, i.e. the C ABI by ctypes, so ROBOSAT_HIP_LIB=/path/to/librobosat_hip.so runs
another build of the library from the same script.  `table` reads each run's kernel trace and prints the average us per launch
side by side; kernel names of a tree where the variants are template arguments are shown under the names of the separate kernels
(`nll_fwd_kernel<2, Px::IgnoreWeight, ...>` as `nll_fwd_pw_kernel<2>`), so the rows line up across the trees."""

import argparse
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IGNORE = 255


def run(args):
    import torch

    from robosat_amd import ops

    dev = "cuda:0"
    n, c, size = 32, args.classes, 512
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(n, c, size, size, generator=gen).to(dev)
    t = torch.randint(0, c, (n, size, size), generator=gen)
    t_ig = t.clone()
    t_ig[torch.rand(n, size, size, generator=gen) < 0.3] = IGNORE
    t, t_ig = t.to(dev), t_ig.to(dev)
    cw = torch.linspace(1.0, 2.0, c).to(dev)
    plane = ops.boundary_weight_plane(t_ig, 4.0, 1.5, ignore=IGNORE, classes=c)
    gout = torch.tensor(1.0, device=dev)
    for _ in range(args.warmup + args.launches):
        for mode in (ops.NLL_CROSS_ENTROPY, ops.NLL_FOCAL):
            _, stats = ops.nll_loss_fwd(x, t_ig, cw, mode, 2.0, ignore=IGNORE, pixel_weight=plane)
            ops.nll_loss_bwd(x, t_ig, cw, stats, gout, mode, 2.0, ignore=IGNORE, pixel_weight=plane)
        ops.lovasz_fwd(x, t)
        ops.lovasz_fwd(x, t_ig, ignore=IGNORE)
        ops.lovasz_softmax_fwd(x, t, per_image=True)
        ops.lovasz_softmax_fwd(x, t_ig, per_image=True, ignore=IGNORE)
    torch.cuda.synchronize()


_VARIANT = (("_pw", ("(Px)2", "Px::IgnoreWeight", "IgnoreAndWeight")), ("_ig", ("(Px)1", "Px::Ignore", "true")), ("", ()))


def label(name):
    """`nll_fwd_pw_kernel<2>` for both `...::nll_fwd_pw_kernel<2>(...)` and `...::nll_fwd_kernel<2, (...Px)2, ...>(...)`."""

    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    m = re.match(r"(\w+?)_kernel(?:<(.*)>)?\(", name) or re.match(r"(\w+?)_kernel(?:<(.*)>)?$", name)
    if not m:
        return name
    base, targs = m.group(1), m.group(2) or ""
    suffix = next(s for s, marks in _VARIANT if not marks or any(k in targs for k in marks))
    ints = re.match(r"\s*(\d+)", targs)
    return "{}{}_kernel{}".format(base, suffix, "<{}>".format(ints.group(1)) if ints else "")


def read_stats(directory):
    """label -> (average us, calls, total us) from the run's rocpd database (rocprofv3's default output) or its kernel_stats.csv."""

    rows = {}
    dbs = glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True)
    if dbs:
        assert len(dbs) == 1, (directory, dbs)
        import sqlite3

        con = sqlite3.connect(dbs[0])
        for name, calls, average, total in con.execute("SELECT name, COUNT(*), AVG(duration), SUM(duration) FROM kernels GROUP BY name"):
            rows[label(name)] = (average / 1e3, calls, total / 1e3)
        return rows
    paths = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    assert len(paths) == 1, (directory, paths)
    with open(paths[0]) as fp:
        for row in csv.DictReader(fp):
            rows[label(row["Name"])] = (float(row["AverageNs"]) / 1e3, int(row["Calls"]), float(row["TotalDurationNs"]) / 1e3)
    return rows


def table(args):
    runs = [spec.split("=", 1) for spec in args.runs]
    stats = [(name, read_stats(path)) for name, path in runs]
    first = stats[0][1]
    print("{:<44}".format("kernel") + "".join("{:>10}".format(name) for name, _ in stats))
    for kernel in sorted(first, key=lambda k: -first[k][2]):
        cells = "".join("{:>10.2f}".format(rows[kernel][0]) if kernel in rows else "{:>10}".format("-") for _, rows in stats)
        print("{:<44}{}  [{}]".format(kernel, cells, first[kernel][1]))
    for name, rows in stats:
        extra = sorted(set(rows) - set(first))
        if extra:
            print("only in {}: {}".format(name, ", ".join(extra)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--classes", type=int, default=2)
    r.add_argument("--launches", type=int, default=20)
    r.add_argument("--warmup", type=int, default=3)
    t = sub.add_parser("table")
    t.add_argument("runs", nargs="+", metavar="NAME=DIR")
    args = ap.parse_args()
    (run if args.cmd == "run" else table)(args)


if __name__ == "__main__":
    main()
