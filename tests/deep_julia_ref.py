"""Deep Julia views (fr_render_deep_julia, fr_render_deepx_julia): ground truth with nothing but Python integers, decimal and
numpy, next to deep_ref / deep_ship_ref / deepx_ref.

- alpha_centre: the fixed point alpha = (1 - sqrt(1 - 4c)) / 2 (principal root) of z^2 + c as decimal strings;
- fixed_orbits / reference_orbits / reference_orbits_x: the header's two orbits P (from the centre) and Q (from 0) in Python
  ints, as doubles and in the extended storage;
- perturb: the kernel's two-orbit step with rebasing onto Q, vectorised over samples in fp64, op for op;
- perturb_x: the same in the two-mode extended arithmetic of deepx_ref, with the flush;
- smooth: nu of the fp64 Julia path;  direct_fp64: fr_render's plain double iteration of a shallow view;
- exact_iter / exact_iter_x: the direct iteration of one sample in fixed point at F + 64 fraction bits (no perturbation).
"""
from __future__ import annotations

import decimal
import functools
import os
from fractions import Fraction

import numpy as np

import deep_ref as R
import deep_ship_ref as S
import deepx_ref as X

X_FLUSH = -(1 << 27)         # a normalised dz with e below this becomes the zero
C_DEFAULT = (float(np.float32(-0.7)), float(np.float32(0.27015)))


def alpha_centre(c, D: int):
    """alpha = (1 - sqrt(1 - 4c)) / 2 with the principal root, at 1300 digits, quantised to D decimals: (cx, cy) strings.
    c = (re, im) doubles, taken exactly."""
    with decimal.localcontext() as ctx:
        ctx.prec = 1300
        Dm = decimal.Decimal
        a = 1 - 4 * Dm(c[0])
        b = -4 * Dm(c[1])
        r = (a * a + b * b).sqrt()
        re = ((r + a) / 2).sqrt()
        im = ((r - a) / 2).sqrt()
        if b < 0:
            im = -im
        q = Dm(1).scaleb(-D)
        ax = ((1 - re) / 2).quantize(q, rounding=decimal.ROUND_HALF_EVEN)
        ay = (-im / 2).quantize(q, rounding=decimal.ROUND_HALF_EVEN)
        return ("0" if ax == 0 else format(ax, "f")), ("0" if ay == 0 else format(ay, "f"))


def _view(name, c, D, zoom, max_iter, F):
    cx, cy = alpha_centre(c, D)
    return dict(name=name, c=c, cx=cx, cy=cy, zoom=zoom, max_iter=max_iter, F=F)


_CACHE = {}


def view(name: str) -> dict:
    """The issue's views.  zoom is a float for the fp64 entry point; zoom_s the same zoom as a string (extended entry point)."""
    if name not in _CACHE:
        spec = {
            "RABBIT30": ((-0.12, 0.74), 45, "1e-30", 1100, 256),
            "DENDRITE30": ((0.0, 1.0), 45, "1e-30", 400, 256),
            "DENDRITE100": ((0.0, 1.0), 115, "1e-100", 1200, 512),
            "DUST30": ((-0.8, 0.156), 45, "1e-30", 1600, 256),
            "BASILICA30": ((-1.0, 0.0), 45, "1e-30", 400, 256),
            "DENDRITE400": ((0.0, 1.0), 420, "1e-400", 3000, 1472),
            "DENDRITE1000": ((0.0, 1.0), 1020, "1e-1000", 7400, 3456),
        }[name]
        c, D, zs, mi, F = spec
        v = _view(name, c, D, float(zs), mi, F)                      # the float is 0.0 below 1e-323: those views are extended only
        v["zoom_s"] = zs
        _CACHE[name] = v
    return _CACHE[name]


SHALLOW = [
    dict(name="shallow0", c=C_DEFAULT, cx="0", cy="0", zoom=3.0, zoom_s="3.0", max_iter=256, F=128),
    dict(name="shallow1", c=C_DEFAULT, cx="-0.5", cy="0.3", zoom=0.2, zoom_s="0.2", max_iter=256, F=128),
    dict(name="shallow2", c=(-1.0, 0.0), cx="0", cy="0", zoom=3.0, zoom_s="3.0", max_iter=256, F=128),
    dict(name="shallow3", c=(-0.12, 0.74), cx="0.25", cy="-0.5", zoom=1.0, zoom_s="1.0", max_iter=256, F=128),
]


def c_fixed(c: float, F: int) -> int:
    """round_half_even(c 2^F): exact wherever F holds the double's last bit"""
    return round(Fraction(c) * (1 << F))


def fixed_orbits(v: dict, bailout: float = 4.0):
    """(P, Q) as lists of Python-int pairs (value 2^F)"""
    F = v["F"]
    Cr, Ci = c_fixed(v["c"][0], F), c_fixed(v["c"][1], F)
    T = Fraction(float(np.float32(bailout)) ** 2) * (1 << (2 * F))
    out = []
    for zr, zi in ((R.parse_fixed(v["cx"], F), R.parse_fixed(v["cy"], F)), (0, 0)):
        pts = [(zr, zi)]
        for _ in range(v["max_iter"]):
            sr, si = zr * zr, zi * zi
            if sr + si > T:
                break
            zr, zi = (sr >> F) - (si >> F) + Cr, ((2 * zr * zi) >> F) + Ci
            pts.append((zr, zi))
        out.append(pts)
    return out[0], out[1]


def reference_orbits(v: dict, bailout: float = 4.0):
    """(P, Q) as (N + 1, 2) float64 arrays (int / int: correctly rounded)"""
    F = v["F"]
    return tuple(np.array([(zr / (1 << F), zi / (1 << F)) for zr, zi in pts], np.float64) for pts in fixed_orbits(v, bailout))


def reference_orbits_x(v: dict, bailout: float = 4.0):
    """((P mant, P exp2), (Q mant, Q exp2)) in the storage of fr_deepx_reference_orbit"""
    out = []
    for pts in fixed_orbits(v, bailout):
        st = [X.store_point(zr, zi, v["F"]) for zr, zi in pts]
        out.append((np.array([(p[0], p[1]) for p in st], np.float64), np.array([p[2] for p in st], np.int32)))
    return out[0], out[1]


def perturb(P: np.ndarray, Q: np.ndarray, d0x: np.ndarray, d0y: np.ndarray, max_iter: int, bailout: float = 4.0):
    """The header's per-sample loop on flat or 2-D sample arrays.  Returns (iter, r2, rebases, moved): moved = the share of
    samples that left P for Q."""
    ox = np.concatenate([Q[:, 0], P[:, 0]])
    oy = np.concatenate([Q[:, 1], P[:, 1]])
    NQ, NP, poff = len(Q) - 1, len(P) - 1, len(Q)
    B2 = np.float64(np.float32(bailout)) * np.float64(np.float32(bailout))
    shape = d0x.shape
    dzx, dzy = d0x.ravel().astype(np.float64).copy(), d0y.ravel().astype(np.float64).copy()
    n = dzx.size
    it = np.full(n, max_iter, np.int32)
    r2out = np.zeros(n, np.float64)
    moved = np.zeros(n, bool)
    idx = np.arange(n)
    m = np.zeros(n, np.int64)
    base = np.full(n, poff, np.int64)
    N = np.full(n, NP, np.int64)
    rebases = 0
    for i in range(max_iter):
        if idx.size == 0:
            break
        Zx, Zy = ox[base + m], oy[base + m]
        tx = (Zx + Zx) + dzx
        ty = (Zy + Zy) + dzy
        nx = tx * dzx - ty * dzy
        ny = tx * dzy + ty * dzx
        m = m + 1
        zx = ox[base + m] + nx
        zy = oy[base + m] + ny
        r2 = zx * zx + zy * zy
        esc = r2 > B2
        reb = ~esc & ((r2 < nx * nx + ny * ny) | (m == N))
        rebases += int(reb.sum())
        moved[idx[reb]] = True
        dzx = np.where(reb, zx, nx)
        dzy = np.where(reb, zy, ny)
        m = np.where(reb, 0, m)
        base = np.where(reb, 0, base)
        N = np.where(reb, NQ, N)
        if esc.any():
            it[idx[esc]] = i
            r2out[idx[esc]] = r2[esc]
            k = ~esc
            idx, dzx, dzy, m, base, N = idx[k], dzx[k], dzy[k], m[k], base[k], N[k]
    return it.reshape(shape), r2out.reshape(shape), rebases, float(moved.mean())


def smooth(it: np.ndarray, r2: np.ndarray, max_iter: int, bailout: float = 4.0) -> np.ndarray:
    """nu of the fp64 Julia path: the ship's form (the two shaders share it)"""
    return S.smooth(it, r2, max_iter, bailout)


def restate(v: dict, W: int, H: int, aa: int = 1, bailout: float = 4.0, rows=None, orbits=None, stats=None):
    """Every sub-sample of the rows: a list over s of (iter, r2) planes"""
    P, Q = orbits if orbits is not None else reference_orbits(v, bailout)
    out = []
    for s in range(aa * aa):
        d0x, d0y = S.sample_dc(W, H, v["zoom"], aa, s, rows)
        it, r2, rb, mv = perturb(P, Q, d0x, d0y, v["max_iter"], bailout)
        if stats is not None:
            stats["rebases"] = stats.get("rebases", 0) + rb
            stats.setdefault("moved", []).append(mv)
        out.append((it, r2))
    return out


def direct_fp64(v: dict, W: int, H: int, bailout: float = 4.0):
    """iter of the plain double iteration z <- z^2 + c from z_0 = centre + d0, update then test (fr_render's Julia loop, aa 1)"""
    d0x, d0y = S.sample_dc(W, H, v["zoom"], 1, 0)
    zx, zy = d0x + np.float64(float(v["cx"])), d0y + np.float64(float(v["cy"]))
    cr, ci = np.float64(v["c"][0]), np.float64(v["c"][1])
    B2 = np.float64(np.float32(bailout)) ** 2
    it = np.full(zx.shape, v["max_iter"], np.int32)
    live = np.ones(zx.shape, bool)
    with np.errstate(all="ignore"):
        for i in range(v["max_iter"]):
            zx, zy = (zx * zx - zy * zy) + cr, (np.float64(2.0) * zx * zy) + ci
            esc = live & (zx * zx + zy * zy > B2)
            it[esc] = i
            live &= ~esc
            zx, zy = np.where(live, zx, 0.0), np.where(live, zy, 0.0)
    return it


def _exact(v: dict, z0r: Fraction, z0i: Fraction, bailout: float) -> int:
    """z <- z^2 + c in Python ints at G = F + 64 fraction bits, update then test.  Three squarings per step: the two squares
    of the escape test are the next step's, and 2 zr zi = (zr + zi)^2 - zr^2 - zi^2 exactly."""
    G = v["F"] + 64
    zr, zi = round(z0r * (1 << G)), round(z0i * (1 << G))
    cr, ci = c_fixed(v["c"][0], G), c_fixed(v["c"][1], G)
    T = Fraction(float(np.float32(bailout)) ** 2) * (1 << (2 * G))
    assert T.denominator == 1
    T = int(T)
    sr, si = zr * zr, zi * zi
    for i in range(v["max_iter"]):
        t = zr + zi
        zr, zi = ((sr - si) >> G) + cr, ((t * t - sr - si) >> G) + ci
        sr, si = zr * zr, zi * zi
        if sr + si > T:
            return i
    return v["max_iter"]


def exact_iter(v: dict, x: int, y: int, W: int, H: int, bailout: float = 4.0) -> int:
    """The escape index of sample (x, y), aa 1, by the direct iteration of z^2 + c from z_0 = centre + d0 (d0 the kernel's
    double, taken exactly)"""
    d0x, d0y = S.sample_dc(W, H, v["zoom"], 1, 0, rows=[y])
    return _exact(v, Fraction(v["cx"]) + Fraction(float(d0x[0, x])), Fraction(v["cy"]) + Fraction(float(d0y[0, x])), bailout)


def exact_iter_x(v: dict, x: int, y: int, W: int, H: int, bailout: float = 4.0) -> int:
    """exact_iter with d0 = (mantissas formed with zm) 2^ze, exact"""
    zm, ze = X.zoom_pair(v["zoom_s"])
    mx, my = S.sample_dc(W, H, zm, 1, 0, rows=[y])
    s = Fraction(2) ** ze
    return _exact(v, Fraction(v["cx"]) + Fraction(float(mx[0, x])) * s, Fraction(v["cy"]) + Fraction(float(my[0, x])) * s, bailout)


# ---- extended deltas ------------------------------------------------------------------------------------------------------
def sample_d0_x(W: int, H: int, zm: float, ze: int, aa: int, s: int, rows=None):
    """(x, y, e) of the first delta of sub-sample s of every pixel of the rows: norm(the ship map's mantissas with zm, ze)"""
    mx, my = S.sample_dc(W, H, zm, aa, s, rows)
    return X._norm(mx.ravel(), my.ravel(), np.full(mx.size, ze, np.int64))


def perturb_x(Px, Qx, d0, max_iter: int, bailout: float = 4.0, stats=None):
    """deepx_ref.perturb_x without a dc term, from dz = d0 on P, rebasing onto Q, with the flush.  Returns (iter, r2)."""
    mant = np.concatenate([Qx[0], Px[0]])
    exp2 = np.concatenate([Qx[1], Px[1]])
    omx, omy = np.ascontiguousarray(mant[:, 0]), np.ascontiguousarray(mant[:, 1])
    oe = exp2.astype(np.int64)
    plain = X.decode(mant, exp2)
    opx, opy = np.ascontiguousarray(plain[:, 0]), np.ascontiguousarray(plain[:, 1])
    NQ, NP, poff = len(Qx[1]) - 1, len(Px[1]) - 1, len(Qx[1])
    B2 = np.float64(np.float32(bailout)) * np.float64(np.float32(bailout))
    _ld, _norm = X._ld, X._norm
    x0, y0, e0 = d0
    n = x0.size
    it = np.full(n, max_iter, np.int32)
    r2out = np.zeros(n, np.float64)
    idx = np.arange(n)
    ext = e0 <= X.X_THR                                            # the mode rule, applied at once
    with np.errstate(all="ignore"):
        dx = np.where(ext, x0, _ld(x0, np.where(ext, 0, e0)))
        dy = np.where(ext, y0, _ld(y0, np.where(ext, 0, e0)))
    ed = e0.astype(np.int64).copy()
    m = np.zeros(n, np.int64)
    base = np.full(n, poff, np.int64)
    N = np.full(n, NP, np.int64)
    n_ext = n_plain = n_reb = n_flush = to_plain = to_ext = 0
    with np.errstate(all="ignore"):
        for i in range(max_iter):
            if idx.size == 0:
                break
            esc = np.zeros(idx.size, bool)
            r2e = np.zeros(idx.size)
            E = np.nonzero(ext)[0]
            P = np.nonzero(~ext)[0]
            if E.size:
                n_ext += E.size
                mm, bb = m[E], base[E]
                Zx, Zy, eZ = omx[bb + mm], omy[bb + mm], oe[bb + mm]
                x, y, e = dx[E], dy[E], ed[E]
                et = np.maximum(eZ + 1, e)
                tx = _ld(Zx, eZ + 1 - et) + _ld(x, e - et)
                ty = _ld(Zy, eZ + 1 - et) + _ld(y, e - et)
                nx = tx * x - ty * y
                ny = tx * y + ty * x
                en = et + e
                mm = mm + 1
                Wx, Wy, eW = omx[bb + mm], omy[bb + mm], oe[bb + mm]
                ez = np.maximum(eW, en)
                zx = _ld(Wx, eW - ez) + _ld(nx, en - ez)
                zy = _ld(Wy, eW - ez) + _ld(ny, en - ez)
                r2 = zx * zx + zy * zy
                r2d = _ld(r2, 2 * ez)
                es = r2d > B2
                n2 = nx * nx + ny * ny
                reb = ~es & ((r2 < _ld(n2, 2 * (en - ez))) | (mm == N[E]))
                n_reb += int(reb.sum())
                ax, ay, ea = _norm(np.where(reb, zx, nx), np.where(reb, zy, ny), np.where(reb, ez, en))
                fl = ea < X_FLUSH
                n_flush += int((fl & (ea != X.X_ZERO) & ~es).sum())
                ax, ay, ea = np.where(fl, 0.0, ax), np.where(fl, 0.0, ay), np.where(fl, X.X_ZERO, ea)
                stay = ea <= X.X_THR
                to_plain += int((~stay & ~es).sum())
                dx[E] = np.where(stay, ax, _ld(ax, np.where(stay, 0, ea)))
                dy[E] = np.where(stay, ay, _ld(ay, np.where(stay, 0, ea)))
                ed[E] = ea
                ext[E] = stay
                m[E] = np.where(reb, 0, mm)
                base[E] = np.where(reb, 0, bb)
                N[E] = np.where(reb, NQ, N[E])
                esc[E] = es
                r2e[E] = r2d
            if P.size:
                n_plain += P.size
                mm, bb = m[P], base[P]
                Zx, Zy = opx[bb + mm], opy[bb + mm]
                x, y = dx[P], dy[P]
                tx = (Zx + Zx) + x
                ty = (Zy + Zy) + y
                nx = tx * x - ty * y
                ny = tx * y + ty * x
                mm = mm + 1
                zx = opx[bb + mm] + nx
                zy = opy[bb + mm] + ny
                r2 = zx * zx + zy * zy
                es = r2 > B2
                reb = ~es & ((r2 < nx * nx + ny * ny) | (mm == N[P]))
                n_reb += int(reb.sum())
                ax = np.where(reb, zx, nx)
                ay = np.where(reb, zy, ny)
                small = np.maximum(np.abs(ax), np.abs(ay)) < X._THR
                to_ext += int((small & ~es).sum())
                bx, by, be = _norm(ax, ay, np.zeros(P.size, np.int64))
                dx[P] = np.where(small, bx, ax)
                dy[P] = np.where(small, by, ay)
                ed[P] = be
                ext[P] = small
                m[P] = np.where(reb, 0, mm)
                base[P] = np.where(reb, 0, bb)
                N[P] = np.where(reb, NQ, N[P])
                esc[P] = es
                r2e[P] = r2
            if esc.any():
                it[idx[esc]] = i
                r2out[idx[esc]] = r2e[esc]
                k = ~esc
                idx, dx, dy, ed, ext, m, base, N = idx[k], dx[k], dy[k], ed[k], ext[k], m[k], base[k], N[k]
    if stats is not None:
        for key, val in (("ext_steps", n_ext), ("plain_steps", n_plain), ("rebases", n_reb), ("flushes", n_flush),
                         ("to_plain", to_plain), ("to_ext", to_ext)):
            stats[key] = stats.get(key, 0) + val
    return it, r2out


def restate_x(v: dict, W: int, H: int, aa: int = 1, bailout: float = 4.0, rows=None, orbits=None, stats=None):
    """Every sub-sample of the rows through the extended restatement: a list over s of (iter, r2) planes"""
    Px, Qx = orbits if orbits is not None else reference_orbits_x(v, bailout)
    zm, ze = X.zoom_pair(v["zoom_s"])
    nrows = H if rows is None else len(rows)
    out = []
    for s in range(aa * aa):
        it, r2 = perturb_x(Px, Qx, sample_d0_x(W, H, zm, ze, aa, s, rows), v["max_iter"], bailout, stats)
        out.append((it.reshape(nrows, W), r2.reshape(nrows, W)))
    return out


def lane_updates(it: np.ndarray, max_iter: int) -> int:
    return int(np.minimum(it.astype(np.int64) + 1, max_iter).sum())


# ---- what the tests share: computed once per session, never changed ---------------------------------------------------------
XW, XH = 48, 36              # the frames of the extended-depth views


@functools.lru_cache(maxsize=None)
def random_pixels(W: int, H: int, n: int = 256):
    rng = np.random.default_rng(99)
    return rng.integers(0, H, n), rng.integers(0, W, n)


@functools.lru_cache(maxsize=None)
def exact_samples(name: str, W: int = 256, H: int = 192):
    """exact iter of the 256 random pixels of a view a double holds"""
    v = view(name)
    ys, xs = random_pixels(W, H)
    return np.array([exact_iter(v, int(x), int(y), W, H) for x, y in zip(xs, ys)])


GOLDEN_CHECKED = 16          # samples of the stored DENDRITE1000 values that exact_samples_x recomputes


@functools.lru_cache(maxsize=None)
def exact_samples_x(name: str):
    """exact iter of the 256 random pixels of an extended view's XW x XH frame.  DENDRITE400: computed (13 ms a sample).
    DENDRITE1000 (130 ms a sample at 3520 bits): the stored values of tests/golden/make_deep_julia_golden.py, every
    256 / GOLDEN_CHECKED-th of them recomputed here and required to be what is stored."""
    v = view(name)
    ys, xs = random_pixels(XW, XH)
    if name != "DENDRITE1000":
        return np.array([exact_iter_x(v, int(x), int(y), XW, XH) for x, y in zip(xs, ys)])
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deep_julia_exact.npz")) as z:
        assert np.array_equal(z["ys"], ys) and np.array_equal(z["xs"], xs)
        ex = z[name].astype(np.int64)
    for k in range(0, len(ex), len(ex) // GOLDEN_CHECKED):
        assert exact_iter_x(v, int(xs[k]), int(ys[k]), XW, XH) == ex[k], k
    return ex


@functools.lru_cache(maxsize=None)
def restated(name: str, aa: int = 1, W: int = 256, H: int = 192):
    """(samples, stats) of the fp64 restatement of a named view or of SHALLOW[int(name)]"""
    v = SHALLOW[int(name)] if name.isdigit() else view(name)
    stats = {}
    return restate(v, W, H, aa, stats=stats), stats


@functools.lru_cache(maxsize=None)
def restated_x(name: str, aa: int = 1, W: int = XW, H: int = XH):
    stats = {}
    return restate_x(view(name), W, H, aa, stats=stats), stats
