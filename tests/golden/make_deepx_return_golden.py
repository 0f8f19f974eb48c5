"""Makes tests/golden/deepx_return_views.json and tests/golden/deepx_return.npz: two views whose lanes fall back from the
plain fp64 mode to the extended one dozens of times each (tests/deepx_return_ref.py), and what the restatements and the
exact iteration give on them at 24 x 18, aa 1.  Own data; about ten CPU-minutes, spread over the machine's cores.  Run from the
repository root:

    python tests/golden/make_deepx_return_golden.py            # writes both files
    python tests/golden/make_deepx_return_golden.py --check    # recomputes and compares with the files that are there

The centre.  c0 = "nucleus201" of deepx_views.json, P = 201, 460 digits.  D = dz_P/dc and lam = prod_{m=1}^{P-1} 2 z_m at c0
(|D| = 1.3515e25, |lam| = 1.6823e25, the minibrot is 1 / |lam D| = 4.40e-51 across).  c0 + kappa / (lam D) is the point of the
minibrot that the point kappa of the whole set renormalises to.  kappa = i is a Misiurewicz point (0, i, i - 1, -i, i - 1, ...:
the second and the fourth iterate coincide), so on the small copy z_{4P} = z_{2P}: Newton runs on g(c) = z_{4P}(c) - z_{2P}(c),
g' = D_{4P} - D_{2P}, from c0 + i / (lam D), until |step| < 1e-400.  400 significant digits are written.

Why the lanes return.  Next to a minibrot of period P the reference orbit comes back to about 1 / |D| once per period.  A lane's
dz grows to about |dc| |D| within the period and collapses to about |dc| at its end: above 2^-400 and below it again, once per
period, for as long as the lane lives.

RET130: zoom 1e-130, fr_render_deep renders it too.  RET320: zoom 1e-320, below the double range, F = 1216.

The npz (all 24 x 18, aa 1; <V> is RET130 or RET320):
  ys, xs              the 64 pixels of RET320's exact values: the four corners, then 60 of default_rng(320)
  RET130_exact        exact_iter_x of every pixel             RET320_exact       ... of the 64 pixels
  RET130_px_exact     deepx_phoenix_ref.exact_iter_x (p = r = 0: the bailout is 2) of every pixel; RET320_px_exact: of the 64
  <V>_iter, _r2       deepx_ref.restate_x                     <V>_stats          its stats, in the order of stats_keys
  <V>_bla_iter, _bla_r2, _bla_counts                          deepx_bla_ref.restate_x_bla
  <V>_de_iter, _de_r2, _de_Dx, _de_Dy, _de_eD                 deepx_de_ref.restate_x_de, bla False
  <V>_debla_iter, ... _debla_eD, _debla_counts                deepx_de_ref.restate_x_de, bla True
  <V>_px_iter, _px_zx, _px_zy                                 deepx_phoenix_ref.samples_x with p = r = 0
"""
import concurrent.futures as cf
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import deepx_bla_ref as XB  # noqa: E402
import deepx_de_ref as XD  # noqa: E402
import deepx_phoenix_ref as PX  # noqa: E402
import deepx_ref as X  # noqa: E402

W, H = 24, 18
P = 201
SPECS = {"RET130": ("1e-130", 50000), "RET320": ("1e-320", 152000)}
STATS_KEYS = ("ext_steps", "plain_steps", "to_plain", "to_ext", "rebases")


def centre():
    import mpmath as mp
    mp.mp.dps = 460
    c0s = X.views()["nucleus201"]
    c0 = mp.mpc(mp.mpf(c0s["cx"]), mp.mpf(c0s["cy"]))
    z, lam, D = mp.mpc(0), mp.mpc(1), mp.mpc(0)
    for m in range(P):
        D = 2 * z * D + 1
        if m >= 1:
            lam *= 2 * z
        z = z * z + c0
    print("|z_P(c0)|", mp.nstr(abs(z), 5), "|D|", mp.nstr(abs(D), 5), "|lam|", mp.nstr(abs(lam), 5), "size",
          mp.nstr(1 / abs(lam * D), 5), flush=True)
    c = c0 + mp.mpc(0, 1) / (lam * D)
    for k in range(12):
        z = d = mp.mpc(0)
        at = {}
        for m in range(1, 4 * P + 1):
            d = 2 * z * d + 1
            z = z * z + c
            if m in (2 * P, 4 * P):
                at[m] = (z, d)
        step = (at[4 * P][0] - at[2 * P][0]) / (at[4 * P][1] - at[2 * P][1])
        c -= step
        print("newton", k, "|step|", mp.nstr(abs(step), 3), flush=True)
        if abs(step) < mp.mpf(10) ** -400:
            break
    else:
        raise SystemExit("Newton did not converge")
    fmt = dict(strip_zeros=False, min_fixed=-mp.inf, max_fixed=mp.inf)
    return mp.nstr(c.real, 400, **fmt), mp.nstr(c.imag, 400, **fmt)


def pixels320():
    rng = np.random.default_rng(320)
    ys = np.concatenate([[0, 0, H - 1, H - 1], rng.integers(0, H, 60)]).astype(np.int32)
    xs = np.concatenate([[0, W - 1, 0, W - 1], rng.integers(0, W, 60)]).astype(np.int32)
    return ys, xs


# ---- the jobs: each returns (key, array) pairs; a process each ------------------------------------------------------------------
def job_exact(name, v, phoenix, first, pix):
    """the pixels pix (the chunk that starts at index first of the view's list)"""
    fn = PX.exact_iter_x if phoenix else X.exact_iter_x
    vv = dict(v, p=0.0, r=0.0) if phoenix else v
    return [("%s%s_exact@%d" % (name, "_px" if phoenix else "", first), np.array([fn(vv, x, y, W, H) for y, x in pix], np.int32))]


def job_restate(name, v):
    st = {}
    it, r2 = X.restate_x(v, W, H, stats=st)[0]
    return [(name + "_iter", it), (name + "_r2", r2), (name + "_stats", np.array([st[k] for k in STATS_KEYS], np.int64))]


def job_bla(name, v):
    s, counts = XB.restate_x_bla(v, W, H)
    return [(name + "_bla_iter", s[0][0]), (name + "_bla_r2", s[0][1]), (name + "_bla_counts", np.array(counts, np.int64))]


def job_de(name, v, bla):
    s, counts = XD.restate_x_de(v, W, H, bla=bla)
    tag = name + ("_debla_" if bla else "_de_")
    out = [(tag + k, a) for k, a in zip(("iter", "r2", "Dx", "Dy", "eD"), s[0])]
    return out + ([(tag + "counts", np.array(counts, np.int64))] if bla else [])


def job_px(name, v):
    it, _, zx, zy = PX.samples_x(dict(v, p=0.0, r=0.0), W, H)[0]
    return [(name + "_px_iter", it), (name + "_px_zx", zx), (name + "_px_zy", zy)]


def _timed(fn, *a):
    t = time.time()
    out = fn(*a)
    print("%-12s %-7s %6.1f s" % (fn.__name__, a[0], time.time() - t), flush=True)
    return out


def main(check):
    cx, cy = centre()
    views = {n: dict(cx=cx, cy=cy, zoom=z, max_iter=mi) for n, (z, mi) in SPECS.items()}
    ys, xs = pixels320()
    pix = {"RET130": [(y, x) for y in range(H) for x in range(W)], "RET320": [(int(y), int(x)) for y, x in zip(ys, xs)]}
    jobs = []
    for name in ("RET320", "RET130"):                             # the long ones first
        v = views[name]
        jobs += [(job_restate, name, v), (job_de, name, v, False), (job_de, name, v, True), (job_bla, name, v), (job_px, name, v)]
    for name, chunk in (("RET320", 8), ("RET130", 72)):
        for ph in (False, True):
            jobs += [(job_exact, name, views[name], ph, k, pix[name][k:k + chunk]) for k in range(0, len(pix[name]), chunk)]
    data = {"ys": ys, "xs": xs, "stats_keys": np.array(STATS_KEYS)}
    parts = {}
    with cf.ProcessPoolExecutor(max_workers=min(os.cpu_count() or 1, 16)) as ex:
        for res in [f.result() for f in [ex.submit(_timed, *j) for j in jobs]]:
            for key, arr in res:
                if "@" in key:
                    base, first = key.split("@")
                    parts.setdefault(base, []).append((int(first), arr))
                else:
                    data[key] = arr
    for base, chunks in parts.items():
        flat = np.concatenate([a for _, a in sorted(chunks, key=lambda c: c[0])])
        data[base] = flat.reshape(H, W) if base.startswith("RET130") else flat
    for name, v in views.items():
        st = dict(zip(STATS_KEYS, data[name + "_stats"].tolist()))
        it = data[name + "_iter"]
        ex = data[name + "_exact"]
        mine = it if name == "RET130" else it[ys, xs]
        print(name, "F", X.frac_bits_x(v["zoom"]), st, "to_ext per lane %.1f" % (st["to_ext"] / (W * H)), "bla counts",
              data[name + "_bla_counts"].tolist(), "distinct escape indices", len(np.unique(it[it < v["max_iter"]])), "range",
              int(it.min()), int(it[it < v["max_iter"]].max()), "interior", int((it == v["max_iter"]).sum()),
              "largest class %.3f" % (np.unique(it, return_counts=True)[1].max() / it.size),
              "restated != exact", int((mine != ex).sum()), "of", ex.size,
              "bla != plain iter", int((data[name + "_bla_iter"] != it).sum()), flush=True)
    jpath, zpath = os.path.join(HERE, "deepx_return_views.json"), os.path.join(HERE, "deepx_return.npz")
    if check:
        with open(jpath) as f:
            assert json.load(f) == views, "deepx_return_views.json differs"
        with np.load(zpath) as z:
            assert sorted(z.files) == sorted(data), (sorted(z.files), sorted(data))
            for k in z.files:
                assert z[k].dtype == data[k].dtype and np.array_equal(z[k].view(np.uint8) if z[k].dtype.kind == "f" else z[k],
                                                                      data[k].view(np.uint8) if data[k].dtype.kind == "f" else data[k]), k
        print("both files reproduced")
        return
    with open(jpath, "w") as f:
        json.dump(views, f, indent=1)
        f.write("\n")
    np.savez_compressed(zpath, **data)


if __name__ == "__main__":
    main("--check" in sys.argv[1:])
