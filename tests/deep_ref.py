"""Deep Mandelbrot views (fr_render_deep): ground truth with nothing but Python integers and numpy.

- parse_fixed / frac_bits / reference_orbit: the header's fixed-point reference orbit, in Python ints;
- restate: the kernel's per-sample perturbation step with rebasing, vectorised over samples in fp64, op for op;
- exact_iter: the direct z^2 + c iteration of one sample in fixed point at F + 64 fraction bits (no perturbation at all).
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

# The views of the tests: the default view, and two views far below double precision.  A and B sit next to the
# Misiurewicz point M_{3,1} = -0.10109636384562216... + 0.95628651080914150...i (z_3 = -z_4, z_4 a repelling fixed point;
# found by Newton's method on z_5(c) - z_4(c) = 0 at 150 digits), offset by (0.071, 0.043) view heights so that the
# point lies inside the frame.  Around it the set is a dendrite, self-similar, and the escape counts of a frame spread
# over some 60 values; max_iter is set where 85 % of the samples escape.  A's reference escapes (N = 254 < 256).
SHALLOW = dict(cx="-0.5", cy="0", zoom=3.0, max_iter=256)
VIEW_A = dict(cx="-0.1010963638456221610257854457385515654638", cy="0.9562865108091415007710960577300204358098",
              zoom=1e-30, max_iter=256)
VIEW_B = dict(cx="-0.1010963638456221610257854457386225654638054428262534838769311776607808407404705842748212198105167790263045319086",
              cy="0.9562865108091415007710960577299774358098333365105291700343143215005246590657167325269784107873398072086444724926",
              zoom=1e-100, max_iter=824)
VIEWS = {"shallow": SHALLOW, "A": VIEW_A, "B": VIEW_B}


def frac_bits(zoom: float) -> int:
    bits = 64 + int(-math.log10(zoom) * 3.32) + 64
    bits = min(max(bits, 128), 4096)
    return (bits + 63) // 64 * 64


def parse_fixed(s: str, F: int) -> int:
    """round_half_even(value * 2^F) of a decimal string"""
    return round(Fraction(s) * (1 << F))


def reference_orbit(cx: str, cy: str, zoom: float, max_iter: int, bailout: float = 4.0, F: int = 0) -> np.ndarray:
    """Z_0 .. Z_N as an (N + 1, 2) float64 array: the header's fixed-point recurrence in Python ints."""
    F = F or frac_bits(zoom)
    Cr, Ci = parse_fixed(cx, F), parse_fixed(cy, F)
    b2 = float(np.float32(bailout)) ** 2                        # exact: a float squared in double
    T = Fraction(b2) * (1 << (2 * F))
    zr = zi = 0
    out = [(0.0, 0.0)]
    for n in range(max_iter):
        sr, si = zr * zr, zi * zi
        if sr + si > T:
            break
        zr, zi = (sr >> F) - (si >> F) + Cr, ((2 * zr * zi) >> F) + Ci
        out.append((zr / (1 << F), zi / (1 << F)))              # int / int: correctly rounded
    return np.array(out, dtype=np.float64)


def sample_dc(W: int, H: int, zoom: float, aa: int, s: int, rows=None):
    """dc of sub-sample s (sy = s // aa, sx = s % aa) of every pixel of the rows: (rows, W) arrays, op for op the kernel's"""
    rows = np.arange(H) if rows is None else np.asarray(rows)
    sy, sx = divmod(s, aa)
    px = np.arange(W, dtype=np.float64) + np.float64(sx) / np.float64(aa)
    py = rows.astype(np.float64) + np.float64(sy) / np.float64(aa)
    dcx = ((px - 0.5 * np.float64(W)) / np.float64(H)) * np.float64(zoom)
    dcy = ((py - 0.5 * np.float64(H)) / np.float64(H)) * np.float64(zoom)
    return np.broadcast_to(dcx[None, :], (len(rows), W)).copy(), np.broadcast_to(dcy[:, None], (len(rows), W)).copy()


def perturb(orbit: np.ndarray, dcx: np.ndarray, dcy: np.ndarray, max_iter: int, bailout: float = 4.0):
    """The per-sample step with rebasing.  Returns (iter, r2, rebases): iter = the loop index of the escaping update
    (max_iter if none), r2 = |z|^2 there, rebases = the number of rebases performed over all samples."""
    ox, oy = np.ascontiguousarray(orbit[:, 0]), np.ascontiguousarray(orbit[:, 1])
    N = len(orbit) - 1
    B2 = np.float64(np.float32(bailout)) * np.float64(np.float32(bailout))
    shape = dcx.shape
    dcx, dcy = dcx.ravel().astype(np.float64), dcy.ravel().astype(np.float64)
    n = dcx.size
    it = np.full(n, max_iter, np.int32)
    r2out = np.zeros(n, np.float64)
    idx = np.arange(n)
    dzx = np.zeros(n); dzy = np.zeros(n)
    m = np.zeros(n, np.int64)
    cx, cy = dcx.copy(), dcy.copy()
    rebases = 0
    for i in range(max_iter):
        if idx.size == 0:
            break
        Zx, Zy = ox[m], oy[m]
        tx = (Zx + Zx) + dzx
        ty = (Zy + Zy) + dzy
        nx = (tx * dzx - ty * dzy) + cx
        ny = (tx * dzy + ty * dzx) + cy
        m = m + 1
        zx = ox[m] + nx
        zy = oy[m] + ny
        r2 = zx * zx + zy * zy
        esc = r2 > B2
        reb = ~esc & ((r2 < nx * nx + ny * ny) | (m == N))
        rebases += int(reb.sum())
        dzx = np.where(reb, zx, nx)
        dzy = np.where(reb, zy, ny)
        m = np.where(reb, 0, m)
        if esc.any():
            it[idx[esc]] = i
            r2out[idx[esc]] = r2[esc]
            keep = ~esc
            idx, dzx, dzy, m, cx, cy = idx[keep], dzx[keep], dzy[keep], m[keep], cx[keep], cy[keep]
    return it.reshape(shape), r2out.reshape(shape), rebases


def smooth(it: np.ndarray, r2: np.ndarray, max_iter: int, bailout: float = 4.0) -> np.ndarray:
    """nu of the fp64 Mandelbrot path: i + 1 - log2(log2|z|) for an escaped sample, max_iter otherwise.  At bailout <= 1
    the kernel takes the shader's form as written, through the library log: log_zn = log(r2) / 2,
    nu = i + 1 - log(log_zn / ln 2) / ln 2 -- NaN where log_zn < 0 (r2 < 1), +inf where r2 == 1."""
    nu = np.full(it.shape, float(max_iter))
    e = it < max_iter
    with np.errstate(all="ignore"):
        if np.float32(bailout) > np.float32(1.0):
            nu[e] = (it[e] + 1.0) - np.log2(0.5 * np.log2(r2[e]))
        else:
            ln2 = np.log(np.float64(2.0))
            log_zn = np.log(r2[e]) / np.float64(2.0)
            nu[e] = (it[e].astype(np.float64) + 1.0) - np.log(log_zn / ln2) / ln2
    return nu


def restate(view: dict, W: int, H: int, aa: int = 1, bailout: float = 4.0, rows=None, orbit=None):
    """Every sub-sample of the frame: a list over s of (iter, r2) planes, and the total number of rebases"""
    if orbit is None:
        orbit = reference_orbit(view["cx"], view["cy"], view["zoom"], view["max_iter"], bailout)
    out, total = [], 0
    for s in range(aa * aa):
        dcx, dcy = sample_dc(W, H, view["zoom"], aa, s, rows)
        it, r2, rb = perturb(orbit, dcx, dcy, view["max_iter"], bailout)
        out.append((it, r2))
        total += rb
    return out, total


def exact_iter(cx: str, cy: str, x: int, y: int, W: int, H: int, zoom: float, max_iter: int, bailout: float = 4.0,
               aa: int = 1, s: int = 0, F: int = 0) -> int:
    """The escape index of one sample by the direct iteration of z^2 + c in fixed point at F + 64 fraction bits,
    c = centre + dc exactly (then rounded once)"""
    G = (F or frac_bits(zoom)) + 64
    dcx, dcy = sample_dc(W, H, zoom, aa, s, rows=[y])
    cr = round((Fraction(cx) + Fraction(float(dcx[0, x]))) * (1 << G))
    ci = round((Fraction(cy) + Fraction(float(dcy[0, x]))) * (1 << G))
    b2 = float(np.float32(bailout)) ** 2
    T = Fraction(b2) * (1 << (2 * G))
    zr = zi = 0
    for i in range(max_iter):
        zr, zi = ((zr * zr - zi * zi) >> G) + cr, ((2 * zr * zi) >> G) + ci
        if zr * zr + zi * zi > T:
            return i
    return max_iter
