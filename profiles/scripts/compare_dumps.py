"""Compare two `bench.py --dump-outputs` directories output for output: equal after adding 0.0 (which folds -0.0)?  python compare_dumps.py DIR_A DIR_B"""
import os
import sys

import numpy as np

a, b = sys.argv[1:3]
names = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
assert names and names == sorted(f for f in os.listdir(b) if f.endswith(".npy")), "the two dumps hold different outputs"
bad = 0
for n in names:
    x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
    same = x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x + 0, y + 0) and not np.isnan(x.astype(np.float64)).any()
    bad += not same
    if not same:
        print("DIFFERENT", n, x.shape, float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) if x.shape == y.shape else "")
print(f"{len(names)} outputs compared, {bad} differ")
sys.exit(1 if bad else 0)
