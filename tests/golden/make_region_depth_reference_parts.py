#!/usr/bin/env python3
"""Generates tests/golden/region_depth_reference_parts.npz (run from the repo root: python
tests/golden/make_region_depth_reference_parts.py).

Runs the binning test of tests/test_region_depths_cpu.py against the live oracle/_ref/libmld_ref.so (built by `make -C oracle
ref` from the reference's Histogram.cpp) and stores the library's bin counts, keyed by a hash of their inputs, so that the
test can check the restatement against the reference's own object code where that library cannot be built.  Only the
answers are stored, nothing of the reference's sources.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import test_region_depths_cpu as t  # noqa: E402


def main():
    if t.ref is None:
        sys.exit("oracle/_ref/libmld_ref.so is not built: run `make -C oracle ref` first")
    fn = t.test_the_binning_of_box_sized_lists_equals_the_reference_class
    for v in [m for m in fn.pytestmark if m.name == "parametrize"][0].args[1]:
        fn(*v)
    np.savez_compressed(t.GOLDEN, **t.RECORDED)
    print(f"{t.GOLDEN}: {len(t.RECORDED)} answers")


if __name__ == "__main__":
    main()
