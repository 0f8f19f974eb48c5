"""Deep Burning Ship views with extended-exponent deltas (fr_render_deepx_ship): ground truth with nothing but Python
integers and numpy, next to deepx_ref (the extended arithmetic) and deep_ship_ref (the fold, the ship's map and colours).

- fixed_orbit_ship / reference_orbit_x_ship: the ship's fixed-point orbit in the storage of fr_deepx_ship_reference_orbit;
- sample_dc_ship_x: the ship's viewport map on the zoom's mantissa, normalised with the zoom's exponent, and dcp;
- fold_x: the fold in the delta's frame; fold_x_exact: the same quantity as an exact Fraction; fold_x_undoubled: a wrong
  fold that drops the factor 2 of the flipped branch, to show which fixtures notice;
- perturb_ship_x / restate_ship_x: the kernel's two-mode per-sample step, op for op;
- exact_iter_ship_x: the direct iteration of (|x| + i|y|)^2 + c of one sample in fixed point at F + 64 bits.

The views of the tests are data: tests/golden/deepx_ship_views.json (made, with the exact iteration counts of
tests/golden/deepx_ship_exact.npz, by tests/golden/make_deepx_ship_golden.py).
"""
from __future__ import annotations

import json
import os
from fractions import Fraction

import numpy as np

import deep_ref as R
import deep_ship_ref as S
import deepx_ref as X
from deepx_ref import X_THR, X_ZERO, _THR, _ld, _norm

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def views() -> dict:
    with open(os.path.join(_GOLDEN, "deepx_ship_views.json")) as f:
        return json.load(f)


def exact_golden() -> dict:
    with np.load(os.path.join(_GOLDEN, "deepx_ship_exact.npz")) as z:
        return {k: z[k] for k in z.files}


def as_x_view(v: dict) -> dict:
    """a deep_ship_ref view (zoom a double) as an extended one (zoom its shortest decimal string)"""
    return dict(cx=v["cx"], cy=v["cy"], zoom=repr(float(v["zoom"])), max_iter=v["max_iter"])


def fixed_orbit_ship(cx: str, cy: str, F: int, max_iter: int, bailout: float = 4.0):
    """Z_0 .. Z_N as Python integers (value 2^F): deep_ship_ref.reference_orbit's recurrence, points signed"""
    Cr, Ci = R.parse_fixed(cx, F), R.parse_fixed(cy, F)
    T = Fraction(float(np.float32(bailout)) ** 2) * (1 << (2 * F))
    zr = zi = 0
    out = [(0, 0)]
    for _ in range(max_iter):
        sr, si = zr * zr, zi * zi
        if sr + si > T:
            break
        zr, zi = (sr >> F) - (si >> F) + Cr, ((2 * abs(zr) * abs(zi)) >> F) + Ci
        out.append((zr, zi))
    return out


def reference_orbit_x_ship(cx: str, cy: str, F: int, max_iter: int, bailout: float = 4.0):
    pts = [X.store_point(zr, zi, F) for zr, zi in fixed_orbit_ship(cx, cy, F, max_iter, bailout)]
    return np.array([(p[0], p[1]) for p in pts], np.float64), np.array([p[2] for p in pts], np.int32)


def frac_bits_of(view: dict) -> int:
    return view.get("frac_bits") or X.frac_bits_x(view["zoom"])


def orbit_of(view: dict, bailout: float = 4.0):
    return reference_orbit_x_ship(view["cx"], view["cy"], frac_bits_of(view), view["max_iter"], bailout)


def sample_dc_ship_x(W: int, H: int, zm: float, ze: int, aa: int, s: int, rows=None):
    """(cx, cy, ec) of sub-sample s (sx OUTER) of every pixel of the rows, normalised, and the plain mode's dc: the map of
    deep_ship_ref.sample_dc on the zoom's mantissa -- ((uvx - 0.5) * zm) * aspect, (uvy - 0.5) * zm -- with the exponent ze"""
    mx, my = S.sample_dc(W, H, zm, aa, s, rows)
    cx, cy, ec = _norm(mx.ravel(), my.ravel(), np.full(mx.size, ze, np.int64))
    plain = []
    for c in (cx, cy):
        _, k = np.frexp(c)
        big = (c != 0.0) & (k.astype(np.int64) + ec > -1022)
        plain.append(np.where(big, _ld(c, np.where(big, ec, 0)), 0.0))
    return cx, cy, ec, plain[0], plain[1]


def fold_x(Xm, eZ, a, ed):
    """fold_x of the header: (the folded delta as a mantissa at exponent ed, whether the fold flipped a sign)"""
    Xs = _ld(Xm, eZ - ed)
    X2s = _ld(Xm, eZ + 1 - ed)
    w = Xs + a
    d = X2s + a
    pos = Xm >= 0.0
    flip = np.where(pos, ~(w >= 0.0), w > 0.0)
    return np.where(pos, np.where(flip, -d, a), np.where(flip, d, -a)), flip


def fold_x_undoubled(Xm, eZ, a, ed):
    """A WRONG fold_x, for the tests only: the flipped branch forms d = X + a where the step needs 2X + a (what a kernel that
    aligned X2 with X's shift would compute).  A fixture pins the 2X term iff its iter plane changes under this fold."""
    Xs = _ld(Xm, eZ - ed)
    w = Xs + a
    pos = Xm >= 0.0
    flip = np.where(pos, ~(w >= 0.0), w > 0.0)
    return np.where(pos, np.where(flip, -w, a), np.where(flip, w, -a)), flip


def fold_x_exact(Xm: float, eZ: int, a: float, ed: int) -> Fraction:
    """(|X 2^eZ + a 2^ed| - |X 2^eZ|) / 2^ed, exactly"""
    Xv = Fraction(Xm) * Fraction(2) ** (eZ - ed)
    return abs(Xv + Fraction(a)) - abs(Xv)


def perturb_ship_x(mant, exp2, dc, max_iter: int, bailout: float = 4.0, stats=None, fold=None):
    """The two-mode step of the header on flat sample arrays.  Returns (iter, r2).  stats: ext_steps, plain_steps, to_plain,
    to_ext, rebases as deepx_ref.perturb_x counts them, and flipped_ext = the extended steps in which a fold flipped a sign.
    fold: another extended fold in fold_x's place (the tests show with a wrong one that a fixture would notice it)."""
    fold = fold or fold_x
    omx, omy = np.ascontiguousarray(mant[:, 0]), np.ascontiguousarray(mant[:, 1])
    oe = exp2.astype(np.int64)
    plain = X.decode(mant, exp2)
    opx, opy = np.ascontiguousarray(plain[:, 0]), np.ascontiguousarray(plain[:, 1])
    N = len(oe) - 1
    B2 = np.float64(np.float32(bailout)) * np.float64(np.float32(bailout))
    cx, cy, ec, cpx, cpy = dc
    n = cx.size
    it = np.full(n, max_iter, np.int32)
    r2out = np.zeros(n, np.float64)
    idx = np.arange(n)
    dx = np.zeros(n); dy = np.zeros(n)
    ed = np.full(n, X_ZERO, np.int64)
    ext = np.ones(n, bool)
    m = np.zeros(n, np.int64)
    n_ext = n_plain = to_plain = to_ext = n_reb = n_flip = 0
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
                mm = m[E]
                Zx, Zy, eZ = omx[mm], omy[mm], oe[mm]
                x, y, e = dx[E], dy[E], ed[E]
                fx, flx = fold(Zx, eZ, x, e)
                fy, fly = fold(Zy, eZ, y, e)
                n_flip += int((flx | fly).sum())
                et = np.maximum(eZ + 1, e)
                tx = _ld(np.abs(Zx), eZ + 1 - et) + _ld(fx, e - et)
                ty = _ld(np.abs(Zy), eZ + 1 - et) + _ld(fy, e - et)
                px = tx * fx - ty * fy
                py = tx * fy + ty * fx
                ep = et + e
                en = np.maximum(ep, ec[E])
                nx = _ld(px, ep - en) + _ld(cx[E], ec[E] - en)
                ny = _ld(py, ep - en) + _ld(cy[E], ec[E] - en)
                mm = mm + 1
                Wx, Wy, eW = omx[mm], omy[mm], oe[mm]
                ez = np.maximum(eW, en)
                zx = _ld(Wx, eW - ez) + _ld(nx, en - ez)
                zy = _ld(Wy, eW - ez) + _ld(ny, en - ez)
                r2 = zx * zx + zy * zy
                r2d = _ld(r2, 2 * ez)
                es = r2d > B2
                n2 = nx * nx + ny * ny
                reb = ~es & ((r2 < _ld(n2, 2 * (en - ez))) | (mm == N))
                n_reb += int(reb.sum())
                ax, ay, ea = _norm(np.where(reb, zx, nx), np.where(reb, zy, ny), np.where(reb, ez, en))
                stay = ea <= X_THR
                to_plain += int((~stay & ~es).sum())
                dx[E] = np.where(stay, ax, _ld(ax, np.where(stay, 0, ea)))
                dy[E] = np.where(stay, ay, _ld(ay, np.where(stay, 0, ea)))
                ed[E] = ea
                ext[E] = stay
                m[E] = np.where(reb, 0, mm)
                esc[E] = es
                r2e[E] = r2d
            if P.size:
                n_plain += P.size
                mm = m[P]
                Zx, Zy = opx[mm], opy[mm]
                x, y = dx[P], dy[P]
                fx, fy = S.fold(Zx, x), S.fold(Zy, y)
                tx = (np.abs(Zx) + np.abs(Zx)) + fx
                ty = (np.abs(Zy) + np.abs(Zy)) + fy
                nx = (tx * fx - ty * fy) + cpx[P]
                ny = (tx * fy + ty * fx) + cpy[P]
                mm = mm + 1
                zx = opx[mm] + nx
                zy = opy[mm] + ny
                r2 = zx * zx + zy * zy
                es = r2 > B2
                reb = ~es & ((r2 < nx * nx + ny * ny) | (mm == N))
                n_reb += int(reb.sum())
                ax = np.where(reb, zx, nx)
                ay = np.where(reb, zy, ny)
                small = np.maximum(np.abs(ax), np.abs(ay)) < _THR
                to_ext += int((small & ~es).sum())
                bx, by, be = _norm(ax, ay, np.zeros(P.size, np.int64))
                dx[P] = np.where(small, bx, ax)
                dy[P] = np.where(small, by, ay)
                ed[P] = be
                ext[P] = small
                m[P] = np.where(reb, 0, mm)
                esc[P] = es
                r2e[P] = r2
            if esc.any():
                it[idx[esc]] = i
                r2out[idx[esc]] = r2e[esc]
                k = ~esc
                idx, dx, dy, ed, ext, m = idx[k], dx[k], dy[k], ed[k], ext[k], m[k]
                cx, cy, ec, cpx, cpy = cx[k], cy[k], ec[k], cpx[k], cpy[k]
    if stats is not None:
        for key, v in (("ext_steps", n_ext), ("plain_steps", n_plain), ("to_plain", to_plain), ("to_ext", to_ext),
                       ("rebases", n_reb), ("flipped_ext", n_flip)):
            stats[key] = stats.get(key, 0) + v
    return it, r2out


def restate_ship_x(view: dict, W: int, H: int, aa: int = 1, bailout: float = 4.0, rows=None, orbit=None, stats=None,
                   pixels=None, fold=None):
    """Every sub-sample of the rows: a list over s of (iter, r2) planes.  pixels = (ys, xs): those samples only, flat."""
    mant, exp2 = orbit if orbit is not None else orbit_of(view, bailout)
    zm, ze = X.zoom_pair(view["zoom"])
    nrows = H if rows is None else len(rows)
    out = []
    for s in range(aa * aa):
        dc = sample_dc_ship_x(W, H, zm, ze, aa, s, rows)
        if pixels is not None:
            sel = np.asarray(pixels[0]) * W + np.asarray(pixels[1])
            dc = tuple(a[sel] for a in dc)
        it, r2 = perturb_ship_x(mant, exp2, dc, view["max_iter"], bailout, stats, fold)
        out.append((it, r2) if pixels is not None else (it.reshape(nrows, W), r2.reshape(nrows, W)))
    return out


def exact_iter_ship_x(view: dict, x: int, y: int, W: int, H: int, max_iter: int = 0, bailout: float = 4.0) -> int:
    """The escape index of sample (x, y), aa 1, by the direct iteration of (|x| + i|y|)^2 + c in fixed point at F + 64 bits;
    dc = the ship's map on zm, rounded to double as the kernel forms it, times 2^ze exactly"""
    zm, ze = X.zoom_pair(view["zoom"])
    max_iter = max_iter or view["max_iter"]
    G = frac_bits_of(view) + 64
    mx, my = S.sample_dc(W, H, zm, 1, 0, rows=[y])
    s = Fraction(2) ** ze
    cr = round((Fraction(view["cx"]) + Fraction(float(mx[0, x])) * s) * (1 << G))
    ci = round((Fraction(view["cy"]) + Fraction(float(my[0, x])) * s) * (1 << G))
    T = Fraction(float(np.float32(bailout)) ** 2) * (1 << (2 * G))
    zr = zi = 0
    for i in range(max_iter):
        zr, zi = ((zr * zr - zi * zi) >> G) + cr, ((2 * abs(zr) * abs(zi)) >> G) + ci
        if zr * zr + zi * zi > T:
            return i
    return max_iter
