"""Makes tests/golden/deep_julia_exact.npz: the exact fixed-point escape indices (tests/deep_julia_ref.py: exact_iter_x) of
the 256 random samples of default_rng(99) on the 48 x 36 frame of the dendrite at 1e-1000, DENDRITE1000.  Own data; about
half a minute on one CPU thread at F + 64 = 3520 bits, which is why the tests read it instead of computing it (they recompute
some of its samples; the 1e-400 view's 256 samples are computed by the tests themselves).  Run from the repository root:

    python tests/golden/make_deep_julia_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import deep_julia_ref as J  # noqa: E402


def main():
    ys, xs = J.random_pixels(J.XW, J.XH)
    v = J.view("DENDRITE1000")
    ex = np.array([J.exact_iter_x(v, int(x), int(y), J.XW, J.XH) for x, y in zip(xs, ys)], np.int32)
    np.savez(os.path.join(HERE, "deep_julia_exact.npz"), ys=ys.astype(np.int32), xs=xs.astype(np.int32), DENDRITE1000=ex)
    print("DENDRITE1000", ex.min(), ex.max(), "distinct", len(np.unique(ex)), "largest class",
          np.unique(ex, return_counts=True)[1].max() / len(ex))


if __name__ == "__main__":
    main()
