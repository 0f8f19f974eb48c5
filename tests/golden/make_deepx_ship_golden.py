"""Makes tests/golden/deepx_ship_views.json and tests/golden/deepx_ship_exact.npz: the views of the fr_render_deepx_ship tests
and the exact fixed-point escape indices of 256 random samples of the two structured ones (tests/deepx_ship_ref.py:
exact_iter_ship_x).  Own data, a few minutes on one CPU thread; run from the repository root:

    python tests/golden/make_deepx_ship_golden.py

Every view's conditions are checked here before it is written.

S310, S400 -- structured views, found as deep_ship_ref found B: from B's centre, for d = 101 .. 399, the restatement renders
zoom 1e-d on a 16 x 12 grid with max_iter = int(6.5 d) + 100; the interior pixel with an escaped 4-neighbour nearest the
frame centre (none: the pixel of largest iter) gives the next centre, moved by that pixel's exact decimal dc and quantised
to d + 40 decimals.  max_iter = 1 + the q-quantile of the exact escape indices of the 256 samples of default_rng(99) on
128 x 96, q the largest of 0.85, 0.7, 0.5 at which the restatement agrees with the exact iteration on >= 99 % of the
samples, no single count holds more than 60 % of them and >= 10 % escape (later escapers are chaotic in fp64).

TIP400, TIP1000 -- centre (-2, 0): the orbit has Y = 0 exactly, so fold(0, b) flips once for every sample with b < 0, in its
first extended step (after it b >= 0).  With X = 0 the flipped d = 2X + b is b: these views do not see the 2X term.

TIPY300 -- centre (-2, -2e-301) at 1e-300: Y is stored NONZERO, 2^-1000 below X, and of the size of the deltas, so extended
folds flip on a nonzero coordinate and the 2X term of d = 2X + a decides where samples escape.  Checked here: the
restatement with a fold that forms d = X + a (deepx_ship_ref.fold_x_undoubled) gives another iter plane.

NUC546 -- the period-546 nucleus 1.7e-106 from B's centre: Newton in two real variables on Z_546(c) = 0 with the Jacobian
carried along, at 520 digits, written with 480.  Viewed at 1e-400 every sample is interior.
"""
import json
import math
import os
import sys
import time
from decimal import Decimal, getcontext

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import deep_ship_ref as S  # noqa: E402
import deepx_ref as X  # noqa: E402
import deepx_ship_ref as SX  # noqa: E402

W, H = 128, 96                      # the frame of the exact samples
TW, TH = 48, 36                     # the frame of the tip and nucleus checks
SAVE = {310: "S310", 400: "S400"}
T0 = time.time()


def log(*a):
    print("[%4.0fs]" % (time.time() - T0), *a, flush=True)


def search():
    """the centres at 1e-310 and 1e-400"""
    getcontext().prec = 1200
    gw, gh = 16, 12
    cx, cy = Decimal(S.SHIP_B["cx"]), Decimal(S.SHIP_B["cy"])
    out, no_boundary = {}, 0
    for d in range(101, 400):
        v = dict(cx=format(cx, "f"), cy=format(cy, "f"), zoom="1e-%d" % d, max_iter=int(6.5 * d) + 100)
        it = SX.restate_ship_x(v, gw, gh)[0][0]
        ins = it >= v["max_iter"]
        best = None
        for y in range(gh):
            for x in range(gw):
                if not ins[y, x]:
                    continue
                nb = [(y + dy, x + dx) for dy, dx in ((1, 0), (-1, 0), (0, 1), (0, -1)) if 0 <= y + dy < gh and 0 <= x + dx < gw]
                if any(not ins[a, b] for a, b in nb):
                    k = (x - gw / 2) ** 2 + (y - gh / 2) ** 2
                    if best is None or k < best[0]:
                        best = (k, x, y)
        if best is None:
            y, x = map(int, np.unravel_index(np.argmax(it), it.shape))
            no_boundary += 1
        else:
            _, x, y = best
        z = Decimal(10) ** (-d)
        cx = cx + (Decimal(x) / gw - Decimal("0.5")) * z * Decimal(gw) / Decimal(gh)
        cy = cy + (Decimal(y) / gh - Decimal("0.5")) * z
        q = Decimal(10) ** (-(d + 40))
        cx, cy = cx.quantize(q), cy.quantize(q)
        if d % 25 == 0:
            log("search", d, "inside", int(ins.sum()), "levels without a boundary pixel", no_boundary)
        if d + 1 in SAVE:
            out[SAVE[d + 1]] = dict(cx=format(cx, "f"), cy=format(cy, "f"), zoom="1e-%d" % (d + 1))
    log("search done: levels without a boundary pixel", no_boundary)
    return out


def choose_max_iter(name, v, ys, xs):
    depth = int(v["zoom"].split("-")[1])
    cap = int(6.5 * depth * 1.25) + 100
    raw = np.array([SX.exact_iter_ship_x(v, int(x), int(y), W, H, max_iter=cap) for x, y in zip(xs, ys)])
    log(name, "exact indices", int(raw.min()), "..", int(raw.max()))
    for q in (0.85, 0.7, 0.5):
        mi = int(np.sort(raw)[math.ceil(q * len(raw)) - 1]) + 1
        ex = np.minimum(raw, mi).astype(np.int32)
        vv = dict(v, max_iter=mi)
        st = {}
        got = SX.restate_ship_x(vv, W, H, pixels=(ys, xs), stats=st)[0][0]
        agree = float((got == ex).mean())
        share = float(np.unique(ex, return_counts=True)[1].max() / len(ex))
        escaped = float((ex < mi).mean())
        log(name, "q", q, "max_iter", mi, "agreement", agree, "largest share", share, "escaped", escaped, st)
        if agree >= 0.99 and share <= 0.60 and escaped >= 0.10:
            return vv, ex
    raise SystemExit(name + ": no q of 0.85, 0.7, 0.5 meets the conditions")


def tip(zoom, max_iter, cy="0", nsamp=40):
    v = dict(cx="-2", cy=cy, zoom=zoom, max_iter=max_iter)
    st = {}
    it = SX.restate_ship_x(v, TW, TH, stats=st)[0][0]
    rng = np.random.default_rng(5)
    ys, xs = rng.integers(0, TH, nsamp), rng.integers(0, TW, nsamp)
    ex = np.array([SX.exact_iter_ship_x(v, int(x), int(y), TW, TH) for x, y in zip(xs, ys)])
    u, c = np.unique(it, return_counts=True)
    log("tip", cy, zoom, st, "distinct", len(u), "largest share", float(c.max() / it.size), "interior",
        float((it >= max_iter).mean()), "agreement", float((it[ys, xs] == ex).mean()))
    assert np.array_equal(it[ys, xs], ex) and c.max() / it.size <= 0.60 and len(u) >= 4
    assert st["flipped_ext"] > 0 and st["ext_steps"] > st["plain_steps"] and st["to_plain"] > 0
    if cy != "0":                                                  # the flips meet a nonzero coordinate: the 2X term counts
        wrong = SX.restate_ship_x(v, TW, TH, fold=SX.fold_x_undoubled)[0][0]
        changed = int((wrong != it).sum())
        log("tip", cy, zoom, "pixels whose iter changes with d = X + a in the flipped branch:", changed)
        assert changed >= 100
        assert not np.array_equal(wrong[ys, xs], ex)
    return v


def nucleus():
    mp.mp.dps = 520
    a, b = mp.mpf(S.SHIP_B["cx"]), mp.mpf(S.SHIP_B["cy"])
    sg = lambda t: 1 if t >= 0 else -1  # noqa: E731
    for step in range(40):
        x = y = xa = xb = ya = yb = mp.mpf(0)
        for _ in range(546):
            nx, ny = x * x - y * y + a, 2 * abs(x) * abs(y) + b
            nxa, nxb = 2 * x * xa - 2 * y * ya + 1, 2 * x * xb - 2 * y * yb
            nya = 2 * (sg(x) * abs(y) * xa + abs(x) * sg(y) * ya)
            nyb = 2 * (sg(x) * abs(y) * xb + abs(x) * sg(y) * yb) + 1
            x, y, xa, xb, ya, yb = nx, ny, nxa, nxb, nya, nyb
        det = xa * yb - xb * ya
        da, db = (x * yb - xb * y) / det, (xa * y - x * ya) / det
        a, b = a - da, b - db
        if mp.sqrt(da * da + db * db) < mp.mpf(10) ** -500:
            break
    dist = mp.sqrt((a - mp.mpf(S.SHIP_B["cx"])) ** 2 + (b - mp.mpf(S.SHIP_B["cy"])) ** 2)
    fmt = dict(strip_zeros=False, min_fixed=-mp.inf, max_fixed=mp.inf)
    v = dict(cx=mp.nstr(a, 480, **fmt), cy=mp.nstr(b, 480, **fmt), zoom="1e-400", max_iter=1200)
    st = {}
    mant, exp2 = SX.orbit_of(v)
    it = SX.restate_ship_x(v, TW, TH, orbit=(mant, exp2), stats=st)[0][0]
    ex = [SX.exact_iter_ship_x(v, x, y, TW, TH) for x, y in ((3, 5), (40, 30), (24, 18), (10, 33))]
    log("nucleus: Newton steps", step + 1, "distance from B", mp.nstr(dist, 3), st, "min orbit exponent", int(exp2[1:].min()),
        "exact", ex)
    assert (it == v["max_iter"]).all() and ex == [v["max_iter"]] * 4
    assert st["flipped_ext"] > 0 and int(exp2[1:].min()) < -1022
    return v


def main():
    views, exact = {}, {}
    views["TIP400"] = tip("1e-400", 1500)
    views["TIP1000"] = tip("1e-1000", 3600)
    views["TIPY300"] = tip("1e-300", 1200, cy="-2e-301")
    views["NUC546"] = nucleus()
    rng = np.random.default_rng(99)
    ys, xs = rng.integers(0, H, 256), rng.integers(0, W, 256)
    exact["ys"], exact["xs"] = ys.astype(np.int32), xs.astype(np.int32)
    for name, v in search().items():
        views[name], exact[name] = choose_max_iter(name, v, ys, xs)
    with open(os.path.join(HERE, "deepx_ship_views.json"), "w") as f:
        json.dump(views, f, indent=1, sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "deepx_ship_exact.npz"), **exact)
    log("written")


if __name__ == "__main__":
    main()
