"""Views whose lanes fall back from the plain fp64 mode to the extended one (the plain-to-extended block of deep_orbit_x,
deep_orbit_x_bla and the Phoenix loop): the loaders of tests/golden/deepx_return_views.json and tests/golden/deepx_return.npz.
TEST INFRASTRUCTURE ONLY.

RET130 / RET320: a Misiurewicz point of the period-201 minibrot of deepx_views.json ("nucleus201") at zoom 1e-130 and 1e-320.
The reference orbit comes back to about 1 / 1.35e25 once per period, and with it every lane's dz collapses from about
|dc| 1.35e25 to about |dc|: through 2^-400 downwards once per period, some 27 (RET130) and 50 (RET320) times per lane.
tests/golden/make_deepx_return_golden.py made both files and says what each array of the npz is; the GPU tests read the recorded
restatements (RET320's takes most of a CPU-minute) and the host tests recompute parts of them.
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZE = (24, 18)              # W, H of every recorded frame, aa 1
NAMES = ("RET130", "RET320")


@functools.lru_cache(maxsize=None)
def views() -> dict:
    """name -> dict(cx, cy, zoom, max_iter): deepx_ref's form of a view"""
    with open(os.path.join(_GOLDEN, "deepx_return_views.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _npz() -> dict:
    with np.load(os.path.join(_GOLDEN, "deepx_return.npz")) as z:
        out = {k: z[k] for k in z.files}
    for a in out.values():
        a.setflags(write=False)                                    # shared by every test, never changed
    return out


def golden(name: str, key: str) -> np.ndarray:
    """array <name>_<key> of the npz"""
    return _npz()[name + "_" + key]


def stats(name: str) -> dict:
    """the stats dict of deepx_ref.restate_x on the 24 x 18 frame, as recorded"""
    return dict(zip(_npz()["stats_keys"].tolist(), _npz()[name + "_stats"].tolist()))


def exact_pixels(name: str):
    """(ys, xs) of the recorded exact values: every pixel of RET130 in row-major order, the 64 pixels of RET320"""
    if name == "RET130":
        ys, xs = np.divmod(np.arange(SIZE[0] * SIZE[1]), SIZE[0])
        return ys, xs
    return _npz()["ys"], _npz()["xs"]


def exact(name: str, phoenix: bool = False) -> np.ndarray:
    """the exact escape indices at exact_pixels(name), flat: deepx_ref.exact_iter_x, or deepx_phoenix_ref.exact_iter_x with
    p = r = 0 (the bailout 2 of the Phoenix kernels)"""
    return _npz()[name + ("_px_exact" if phoenix else "_exact")].ravel()
