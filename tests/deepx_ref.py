"""Deep Mandelbrot views with extended-exponent deltas (fr_render_deepx): ground truth with nothing but Python integers
and numpy.

- zoom_pair / frac_bits_x: the zoom string as (zm, ze), correctly rounded, from Fraction; the automatic fraction bits;
- reference_orbit_x: the fixed-point reference orbit of deep_ref in the storage of fr_deepx_reference_orbit (mantissa
  pairs and one binary exponent per point); decode: what the plain mode reads;
- perturb_x / restate_x: the kernel's two-mode per-sample step, op for op (numpy frexp / ldexp for the exponents);
- exact_iter_x: deep_ref.exact_iter with dc formed from the (zm, ze) pair as an exact Fraction.

The views of the tests are data: tests/golden/deepx_views.json (made, with the exact iteration counts of
tests/golden/deepx_exact.npz, by tests/golden/make_deepx_golden.py).
"""
from __future__ import annotations

import json
import math
import os
from fractions import Fraction

import numpy as np

import deep_ref as R

X_ZERO = -(1 << 28)          # FR_DEEPX_ZERO_EXP: the exponent of a zero
X_THR = -400                 # extended while max(|dz.x|, |dz.y|) < 2^X_THR
_THR = math.ldexp(1.0, X_THR)
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def views() -> dict:
    with open(os.path.join(_GOLDEN, "deepx_views.json")) as f:
        return json.load(f)


def exact_golden() -> dict:
    with np.load(os.path.join(_GOLDEN, "deepx_exact.npz")) as z:
        return {k: z[k] for k in z.files}


def zoom_pair(s: str):
    """(zm, ze): zm a double in [1, 2) holding the decimal value / 2^ze correctly rounded to 53 bits, ties to even"""
    q = Fraction(s)
    assert q > 0
    ze = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** ze > q:
        ze -= 1
    assert Fraction(2) ** ze <= q < Fraction(2) ** (ze + 1)
    M = round(q / Fraction(2) ** ze * (1 << 52))                 # round(Fraction): ties to even
    if M == 1 << 53:
        M, ze = M >> 1, ze + 1
    return M / (1 << 52), ze


def frac_bits_x(s: str) -> int:
    zm, ze = zoom_pair(s)
    if ze >= -1000 and math.ldexp(zm, ze) >= 1e-290:
        return R.frac_bits(math.ldexp(zm, ze))
    bits = 64 + int(-(math.log10(zm) + ze * math.log10(2.0)) * 3.32) + 64
    bits = min(max(bits, 128), 4096)
    return (bits + 63) // 64 * 64


def fixed_orbit(cx: str, cy: str, F: int, max_iter: int, bailout: float = 4.0):
    """Z_0 .. Z_N as Python integers (value 2^F): deep_ref.reference_orbit's recurrence"""
    Cr, Ci = R.parse_fixed(cx, F), R.parse_fixed(cy, F)
    b2 = float(np.float32(bailout)) ** 2
    T = Fraction(b2) * (1 << (2 * F))
    zr = zi = 0
    out = [(0, 0)]
    for _ in range(max_iter):
        sr, si = zr * zr, zi * zi
        if sr + si > T:
            break
        zr, zi = (sr >> F) - (si >> F) + Cr, ((2 * zr * zi) >> F) + Ci
        out.append((zr, zi))
    return out


def store_point(zr: int, zi: int, F: int):
    """One point in the storage of fr_deepx_reference_orbit: (mx, my, e), value (mx, my) 2^e.  A point whose larger
    component is a normal double has e = 0 and the doubles of fr_deep_reference_orbit; a smaller one has its larger
    mantissa in [0.5, 1); zero has e = X_ZERO."""
    a = max(abs(zr), abs(zi))
    if a == 0:
        return 0.0, 0.0, X_ZERO
    b = a.bit_length() - 1 - F                                     # 2^b <= larger component < 2^(b + 1)
    if b >= -1022:
        return zr / (1 << F), zi / (1 << F), 0                    # int / int: correctly rounded
    e = b + 1
    return zr / (1 << (F + e)), zi / (1 << (F + e)), e


def reference_orbit_x(cx: str, cy: str, F: int, max_iter: int, bailout: float = 4.0):
    pts = [store_point(zr, zi, F) for zr, zi in fixed_orbit(cx, cy, F, max_iter, bailout)]
    mant = np.array([(p[0], p[1]) for p in pts], np.float64)
    return mant, np.array([p[2] for p in pts], np.int32)


def decode(mant: np.ndarray, exp2: np.ndarray) -> np.ndarray:
    """ldexp(mantissa, exponent), rounded to nearest: the doubles of the plain mode"""
    return np.ldexp(mant, exp2.astype(np.intc)[:, None])


def _ld(x, n):
    return np.ldexp(x, np.clip(n, -(1 << 30), 1 << 30).astype(np.intc))


def _norm(x, y, e):
    """the larger mantissa into [0.5, 1); zero gets X_ZERO"""
    mx = np.maximum(np.abs(x), np.abs(y))
    _, k = np.frexp(mx)
    k = k.astype(np.int64)
    return _ld(x, -k), _ld(y, -k), np.where(mx == 0.0, X_ZERO, e + k)


def sample_dc_x(W: int, H: int, zm: float, ze: int, aa: int, s: int, rows=None):
    """(cx, cy, ec) of sub-sample s of every pixel of the rows, normalised, and the plain mode's dc (a component below
    2^-1022 is 0)"""
    mx, my = R.sample_dc(W, H, zm, aa, s, rows)                   # ((p - 0.5 W) / H) * zm: one rounding
    cx, cy, ec = _norm(mx.ravel(), my.ravel(), np.full(mx.size, ze, np.int64))
    plain = []
    for c in (cx, cy):
        _, k = np.frexp(c)
        big = (c != 0.0) & (k.astype(np.int64) + ec > -1022)
        plain.append(np.where(big, _ld(c, np.where(big, ec, 0)), 0.0))
    return cx, cy, ec, plain[0], plain[1]


def perturb_x(mant, exp2, dc, max_iter: int, bailout: float = 4.0, stats=None):
    """The two-mode step of the header on flat sample arrays.  Returns (iter, r2)."""
    omx, omy = np.ascontiguousarray(mant[:, 0]), np.ascontiguousarray(mant[:, 1])
    oe = exp2.astype(np.int64)
    plain = decode(mant, exp2)
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
    n_ext = n_plain = to_plain = to_ext = n_reb = 0
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
                et = np.maximum(eZ + 1, e)
                tx = _ld(Zx, eZ + 1 - et) + _ld(x, e - et)
                ty = _ld(Zy, eZ + 1 - et) + _ld(y, e - et)
                px = tx * x - ty * y
                py = tx * y + ty * x
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
                tx = (Zx + Zx) + x
                ty = (Zy + Zy) + y
                nx = (tx * x - ty * y) + cpx[P]
                ny = (tx * y + ty * x) + cpy[P]
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
                       ("rebases", n_reb)):
            stats[key] = stats.get(key, 0) + v
    return it, r2out


def orbit_of(view: dict, bailout: float = 4.0):
    F = view.get("frac_bits") or frac_bits_x(view["zoom"])
    return reference_orbit_x(view["cx"], view["cy"], F, view["max_iter"], bailout)


def restate_x(view: dict, W: int, H: int, aa: int = 1, bailout: float = 4.0, rows=None, orbit=None, stats=None):
    """Every sub-sample of the rows: a list over s of (iter, r2) planes"""
    mant, exp2 = orbit if orbit is not None else orbit_of(view, bailout)
    zm, ze = zoom_pair(view["zoom"])
    nrows = H if rows is None else len(rows)
    out = []
    for s in range(aa * aa):
        it, r2 = perturb_x(mant, exp2, sample_dc_x(W, H, zm, ze, aa, s, rows), view["max_iter"], bailout, stats)
        out.append((it.reshape(nrows, W), r2.reshape(nrows, W)))
    return out


def exact_iter_x(view: dict, x: int, y: int, W: int, H: int, max_iter: int = 0, bailout: float = 4.0) -> int:
    """The escape index of sample (x, y), aa 1, by the direct iteration of z^2 + c in fixed point at F + 64 bits;
    dc = (fx zm, fy zm) 2^ze with the products rounded to double as the kernel forms them, then exact"""
    zm, ze = zoom_pair(view["zoom"])
    max_iter = max_iter or view["max_iter"]
    G = (view.get("frac_bits") or frac_bits_x(view["zoom"])) + 64
    mx, my = R.sample_dc(W, H, zm, 1, 0, rows=[y])
    s = Fraction(2) ** ze
    cr = round((Fraction(view["cx"]) + Fraction(float(mx[0, x])) * s) * (1 << G))
    ci = round((Fraction(view["cy"]) + Fraction(float(my[0, x])) * s) * (1 << G))
    T = Fraction(float(np.float32(bailout)) ** 2) * (1 << (2 * G))
    zr = zi = 0
    for i in range(max_iter):
        zr, zi = ((zr * zr - zi * zi) >> G) + cr, ((2 * zr * zi) >> G) + ci
        if zr * zr + zi * zi > T:
            return i
    return max_iter
