"""Makes tests/golden/deepx_views.json and tests/golden/deepx_exact.npz: the views of the fr_render_deepx tests and the
exact fixed-point escape indices of 256 random samples of each (tests/deepx_ref.py: exact_iter_x).  Own data, a few
minutes on one CPU thread (view E alone about two); run from the repository root:

    python tests/golden/make_deepx_golden.py

Views: the Misiurewicz point M_{3,1} of deep_ref's views A and B (Newton on z_3(c) + z_4(c) = 0 from
-0.10109636384562216 + 0.95628651080914150 i at depth + 60 digits), centre = M + (0.071, 0.043) * zoom written with
depth + 40 significant digits.  max_iter = 1 + the index by which 85 % of the 256 samples of default_rng(99) on 256 x 192
have escaped.  "nucleus201": the period-201 nucleus of deep_bla_ref's view C (Newton on z_201(c) from M_{3,1} +
(1e-40, 1e-40)), refined at 450 digits and written with 420.
"""
import json
import math
import os
import sys
import time

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import deepx_ref as X  # noqa: E402

W, H = 256, 192
DEPTHS = {"D": 400, "E": 1000, "T110": 110, "T130": 130, "T260": 260, "T280": 280, "T300": 300, "T320": 320}


def misiurewicz(digits):
    mp.mp.dps = digits
    c = mp.mpc("-0.10109636384562216", "0.95628651080914150")
    for _ in range(40):
        z = dz = mp.mpc(0)
        vals = []
        for _k in range(4):
            dz = 2 * z * dz + 1
            z = z * z + c
            vals.append((z, dz))
        f, df = vals[2][0] + vals[3][0], vals[2][1] + vals[3][1]
        step = f / df
        c -= step
        if abs(step) < mp.mpf(10) ** (-(digits - 5)):
            break
    return c


def nucleus(c, period, digits):
    mp.mp.dps = digits
    for _ in range(60):
        z = dz = mp.mpc(0)
        for _k in range(period):
            dz = 2 * z * dz + 1
            z = z * z + c
        step = z / dz
        c -= step
        if abs(step) < mp.mpf(10) ** (-(digits - 5)):
            break
    return c


def main():
    views, exact = {}, {}
    rng = np.random.default_rng(99)
    ys, xs = rng.integers(0, H, 256), rng.integers(0, W, 256)
    exact["ys"], exact["xs"] = ys.astype(np.int32), xs.astype(np.int32)
    for name, depth in DEPTHS.items():
        M = misiurewicz(depth + 60)
        zoom = mp.mpf(10) ** (-depth)
        cx = mp.nstr(M.real + mp.mpf("0.071") * zoom, depth + 40, strip_zeros=False, min_fixed=-mp.inf, max_fixed=mp.inf)
        cy = mp.nstr(M.imag + mp.mpf("0.043") * zoom, depth + 40, strip_zeros=False, min_fixed=-mp.inf, max_fixed=mp.inf)
        v = dict(cx=cx, cy=cy, zoom="1e-%d" % depth)
        cap = int(depth * 8.1 * 1.25) + 100
        t0 = time.time()
        raw = np.array([X.exact_iter_x(v, int(x), int(y), W, H, max_iter=cap) for x, y in zip(xs, ys)])
        q = int(np.sort(raw)[math.ceil(0.85 * len(raw)) - 1])
        v["max_iter"] = q + 1
        ex = np.minimum(raw, v["max_iter"]).astype(np.int32)
        views[name], exact[name] = v, ex
        print(name, v["zoom"], X.zoom_pair(v["zoom"]), "F", X.frac_bits_x(v["zoom"]), "max_iter", v["max_iter"], "distinct",
              len(np.unique(ex)), "largest share", np.unique(ex, return_counts=True)[1].max() / len(ex), "escaped",
              float((ex < v["max_iter"]).mean()), "secs %.1f" % (time.time() - t0), flush=True)
    M = misiurewicz(460)
    c = nucleus(M + mp.mpc("1e-40", "1e-40"), 201, 450)
    views["nucleus201"] = dict(cx=mp.nstr(c.real, 420, strip_zeros=False, min_fixed=-mp.inf, max_fixed=mp.inf),
                               cy=mp.nstr(c.imag, 420, strip_zeros=False, min_fixed=-mp.inf, max_fixed=mp.inf))
    with open(os.path.join(HERE, "deepx_views.json"), "w") as f:
        json.dump(views, f, indent=1)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "deepx_exact.npz"), **exact)


if __name__ == "__main__":
    main()
