#!/usr/bin/env python3
"""Generate tests/golden/ref_vectors.npz: every output of the REAL reference (oracle/_ref/libref.so) that
tests/test_oracle_vs_ref.py uses, on exactly the inputs of its tests (each test is run once, parametrised cases
included, with the module's RECORD switched on).  Needs oracle/_ref, i.e. the reference sources:

    make -C oracle ref && python tests/golden/make_golden_ref.py

The outputs are plain data (partitions, thresholds, footprints, digests of products); no reference source is stored.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import pyoracle as po  # noqa: E402
import test_oracle_vs_ref as t  # noqa: E402


def main():
    if not po.have_ref():
        raise SystemExit("oracle/_ref/libref.so is not built: make -C oracle ref")
    t.RECORD = {}
    for name, fn in sorted(vars(t).items()):
        if not name.startswith("test_"):
            continue
        marks = [mk for mk in getattr(fn, "pytestmark", []) if mk.name == "parametrize"]
        if not marks:
            fn()
            continue
        argnames, values = marks[0].args
        names = [a.strip() for a in argnames.split(",")]
        for v in values:
            fn(**dict(zip(names, v if len(names) > 1 else (v,))))
    out = os.path.join(HERE, "ref_vectors.npz")
    np.savez_compressed(out, **t.RECORD)
    print(f"{out}: {len(t.RECORD)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
