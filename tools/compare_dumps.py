#!/usr/bin/env python3
"""Compare two bench.py --dump-outputs directories file by file: byte-identical, or max abs diff over the first's max abs.
   tools/compare_dumps.py LABEL DIR_A DIR_B"""
import os
import sys

import numpy as np

label, a, b = sys.argv[1:4]
for f in sorted(os.listdir(a)):
    if not f.endswith(".npy"):
        continue
    x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
    if x.shape == y.shape and x.tobytes() == y.tobytes():
        print(f"{label} {f} byte-identical {x.shape}")
    else:
        d = np.abs(x.astype(np.float64) - y).max() / max(np.abs(x).max(), 1e-30)
        print(f"{label} {f} max abs diff / max|first| = {d:.3e} {x.shape}")
