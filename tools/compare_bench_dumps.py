#!/usr/bin/env python3
"""Are the outputs of two builds the same, bit for bit?  Compares the arrays
two `bench.py --dump-outputs DIR` runs wrote (per Newton batch the nodes and
the active set, and loop_stats), name by name.
    compare_bench_dumps.py DIR_A DIR_B
Exit status 0 only if both hold the same names and every array is identical."""
import glob
import os
import sys

import numpy as np


def main(a_dir, b_dir):
    names = [sorted(os.path.basename(f) for f in glob.glob(os.path.join(d, "*.npy")))
             for d in (a_dir, b_dir)]
    if names[0] != names[1] or not names[0]:
        print("different (or no) arrays: %d in %s, %d in %s"
              % (len(names[0]), a_dir, len(names[1]), b_dir))
        return 1
    differing = 0
    for n in names[0]:
        a, b = np.load(os.path.join(a_dir, n)), np.load(os.path.join(b_dir, n))
        same = a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
        if not same:
            differing += 1
            where = "shape / dtype" if a.shape != b.shape or a.dtype != b.dtype \
                else "%d entries, max |a - b| = %.3g" % (int(np.sum(a != b)),
                                                         float(np.nanmax(np.abs(a - b))))
            print("DIFFERENT %s: %s" % (n, where))
    print("%d arrays, %d identical, %d different" % (len(names[0]), len(names[0]) - differing,
                                                     differing))
    return 1 if differing else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
