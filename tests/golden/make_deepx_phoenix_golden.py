#!/usr/bin/env python3
"""Writes tests/golden/deepx_phoenix_exact.npz: exact_frame_x of every new view of tests/deepx_phoenix_ref.py at 24x18, the
direct fixed-point iteration at F + 64 bits (10 to 40 s per view).  usage: make_deepx_phoenix_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import deepx_phoenix_ref as PX  # noqa: E402

if __name__ == "__main__":
    W, H = PX.GOLDEN_SIZE
    frames = {}
    for name, view in PX.NEW_VIEWS.items():
        frames[name] = PX.exact_frame_x(view, W, H)
        it = frames[name]
        print(name, "distinct", len(np.unique(it[it < view["max_iter"]])), "interior", int((it == view["max_iter"]).sum()), "/", it.size)
    np.savez_compressed(os.path.join(HERE, "deepx_phoenix_exact.npz"), **frames)
