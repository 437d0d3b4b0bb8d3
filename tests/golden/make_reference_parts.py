#!/usr/bin/env python3
"""Generates tests/golden/reference_parts.npz (run from the repo root: python tests/golden/make_reference_parts.py).

Runs every test of tests/test_reference_parts.py against the live oracle/_ref/libmld_ref.so (built by `make -C oracle ref`
from the reference's Histogram.cpp and TresholdDepthGlobal.cpp) and stores the library's answers, keyed by a hash of their
inputs, so that the tests can check the restatement against the reference's own object code where that library cannot be
built.  Only the answers are stored (bin counts, threshold results and depths), nothing of the reference's sources.
"""
import inspect
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from tests import test_reference_parts as t  # noqa: E402


def main():
    if t.ref is None:
        sys.exit("oracle/_ref/libmld_ref.so is not built: run `make -C oracle ref` first")
    for name, fn in inspect.getmembers(t, inspect.isfunction):
        if not name.startswith("test_"):
            continue
        marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
        if not marks:
            fn()
            continue
        argnames, values = marks[0].args
        argnames = [a.strip() for a in argnames.split(",")]
        for v in values:
            fn(*(v if len(argnames) > 1 else (v,)))
    np.savez_compressed(t.GOLDEN, **t.RECORDED)
    print(f"{t.GOLDEN}: {len(t.RECORDED)} answers")


if __name__ == "__main__":
    main()
