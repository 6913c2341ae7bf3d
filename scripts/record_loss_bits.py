#!/usr/bin/env python
"""Writes tests/golden/loss_bits.json: SHA-256 digests of the raw output bytes (loss, stats, gradient, probabilities) of every
entry point of csrc/loss.hip and csrc/lovasz.hip on the fixed inputs of tests/loss_bits_cases.py.  Run on the MI355X with the
library built from the commit whose bits are to be pinned; tests/test_gpu_loss_bits.py then holds every later build to them.

    python scripts/record_loss_bits.py [--commit HASH] [--out tests/golden/loss_bits.json]

One process, one device; --commit names the commit where the tree has no .git (default: git rev-parse HEAD)."""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _first_line(cmd):
    return subprocess.run(cmd, cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip().split("\n")[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "loss_bits.json"))
    args = ap.parse_args()

    import torch

    import loss_bits_cases as cases
    from robosat_amd import _lib

    assert torch.cuda.is_available(), "the digests are of the MI355X's outputs"
    record = {
        "commit": args.commit or _first_line(["git", "rev-parse", "HEAD"]),
        "compiler": _first_line([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"]),
        "kernel_source_digest": _lib.kernel_source_digest(),
        "device": torch.cuda.get_device_name(0),
        "shapes": {},
    }
    total = 0
    for shape in cases.SHAPES:
        got = cases.run_shape(shape)
        torch.cuda.synchronize()
        record["shapes"][cases.shape_key(shape)] = got
        total += len(got)
        print("{:<14} {} cases".format(cases.shape_key(shape), len(got)), flush=True)
    with open(args.out, "w") as fp:
        json.dump(record, fp, indent=0, sort_keys=True)
        fp.write("\n")
    print("{} cases -> {}".format(total, args.out))


if __name__ == "__main__":
    main()
