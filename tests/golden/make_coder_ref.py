#!/usr/bin/env python3
"""Store what the reference's own C++ coder returns on the inputs of test_oracle_coder.py's *_against_reference_cpp tests.

    make -C oracle ref && python tests/golden/make_coder_ref.py

Output (data only -- the inputs are regenerated from seeds by tests/coder_cases.py, never stored):
    tests/golden/coder_ref_cpp.npz  rANS streams of the seeded / lane-edge / coarse-edge cases, the symbols the reference's
                                    decoder returns from them, and its quantised CDFs of the seeded cases' pmfs

All integer work: machine independent.  Where oracle/_ref is built the tests also recompute these and compare.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from coder_cases import reference_cpp_vectors  # noqa: E402
from oracle import coder  # noqa: E402


def main():
    ref = coder.load_reference_coder()
    if ref is None:
        sys.exit("oracle/_ref is not built: run `make -C oracle ref` first")
    kat = dict(np.load(os.path.join(HERE, "coder_kat.npz")))
    gc = coder.Tables(kat["gc_cdf"], kat["gc_sizes"], kat["gc_offsets"])
    out = reference_cpp_vectors(ref, kat["scale_table"], gc)
    path = os.path.join(HERE, "coder_ref_cpp.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
