"""Deep Burning Ship views (fr_render_deep_ship): ground truth with nothing but Python integers and numpy, next to deep_ref.

- reference_orbit: the header's fixed-point orbit of z <- (|x| + i|y|)^2 + c, in Python ints;
- sample_dc: the Burning Ship shader's viewport map less the centre (sx outer), op for op the kernel's;
- fold / perturb: the kernel's per-sample step with rebasing, vectorised over samples in fp64, op for op;
- smooth: nu of the fp64 Burning Ship path;
- exact_iter: the direct iteration of one sample in fixed point at F + 64 fraction bits (no perturbation at all).
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import deep_ref as R

# SHIP_A / SHIP_B: found by repeated 10x zooms onto boundary pixels of a mini-ship on the needle, with exact integer
# iteration.  A's reference escapes (N = 197 < 200); B's does not (N = 590: the orbit ends by m == N).  max_iter is kept
# where fp64 perturbation still agrees with the exact iteration: later escapers are chaotic in fp64.
SHALLOW = dict(cx="-0.5", cy="-0.5", zoom=3.0, max_iter=256)
NEEDLE = dict(cx="-1.75", cy="-0.03", zoom=0.2, max_iter=256)
SHIP_A = dict(cx="-1.786920552661164048615923928484846562729679", cy="-0.011684720658366696321592422425265984253595",
              zoom=1e-30, max_iter=200)
SHIP_B = dict(cx="-1.7869205526611640486159239284847187869255146120455847107521574413273286760371700122867767078216196037388941103258",
              cy="-0.0116847206583666963215924224251631799129266538431655976625957927966982324272073515570780263271063282763864283872",
              zoom=1e-100, max_iter=590)
VIEWS = {"shallow": SHALLOW, "needle": NEEDLE, "A": SHIP_A, "B": SHIP_B}


def reference_orbit(cx: str, cy: str, zoom: float, max_iter: int, bailout: float = 4.0, F: int = 0) -> np.ndarray:
    """Z_0 .. Z_N as an (N + 1, 2) float64 array: Im = floor(2 |Zr| |Zi| / 2^F) + Ci, Re as Mandelbrot's"""
    F = F or R.frac_bits(zoom)
    Cr, Ci = R.parse_fixed(cx, F), R.parse_fixed(cy, F)
    b2 = float(np.float32(bailout)) ** 2
    T = Fraction(b2) * (1 << (2 * F))
    zr = zi = 0
    out = [(0.0, 0.0)]
    for n in range(max_iter):
        sr, si = zr * zr, zi * zi
        if sr + si > T:
            break
        zr, zi = (sr >> F) - (si >> F) + Cr, ((2 * abs(zr) * abs(zi)) >> F) + Ci
        out.append((zr / (1 << F), zi / (1 << F)))
    return np.array(out, dtype=np.float64)


def sample_dc(W: int, H: int, zoom: float, aa: int, s: int, rows=None):
    """dc of sub-sample s (sx = s // aa OUTER, sy = s % aa) of every pixel of the rows: (rows, W) arrays"""
    rows = np.arange(H) if rows is None else np.asarray(rows)
    f = np.float64
    sx, sy = divmod(s, aa)
    uvx = np.arange(W, dtype=f) / f(W)
    uvy = rows.astype(f) / f(H)
    if aa > 1:
        pixel_size = f(1.0) / f(W)
        sample_offset = pixel_size / f(aa)
        centre = sample_offset * f(aa - 1) * f(0.5)
        uvx = uvx + (f(sx) * sample_offset - centre) / f(W)
        uvy = uvy + (f(sy) * sample_offset - centre) / f(H)
    aspect = f(W) / f(H)
    dcx = (uvx - f(0.5)) * f(zoom) * aspect
    dcy = (uvy - f(0.5)) * f(zoom)
    return np.broadcast_to(dcx[None, :], (len(rows), W)).copy(), np.broadcast_to(dcy[:, None], (len(rows), W)).copy()


def fold(X: np.ndarray, a: np.ndarray) -> np.ndarray:
    """|X + a| - |X| from the signs of X and of w = X + a"""
    w = X + a
    d = (X + X) + a
    return np.where(X >= 0.0, np.where(w >= 0.0, a, -d), np.where(w > 0.0, d, -a))


def perturb(orbit: np.ndarray, dcx: np.ndarray, dcy: np.ndarray, max_iter: int, bailout: float = 4.0):
    """deep_ref.perturb with the Burning Ship step.  Returns (iter, r2, rebases, folded): folded = the steps in which a
    fold took a branch other than (a, b) of a non-negative orbit point or (-a, -b) of a negative one."""
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
    rebases = folded = 0
    for i in range(max_iter):
        if idx.size == 0:
            break
        Zx, Zy = ox[m], oy[m]
        fx, fy = fold(Zx, dzx), fold(Zy, dzy)
        folded += int(((np.abs(fx) != np.abs(dzx)) | (np.abs(fy) != np.abs(dzy))).sum())
        tx = (np.abs(Zx) + np.abs(Zx)) + fx
        ty = (np.abs(Zy) + np.abs(Zy)) + fy
        nx = (tx * fx - ty * fy) + cx
        ny = (tx * fy + ty * fx) + cy
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
    return it.reshape(shape), r2out.reshape(shape), rebases, folded


def smooth(it: np.ndarray, r2: np.ndarray, max_iter: int, bailout: float = 4.0) -> np.ndarray:
    """nu of the fp64 Burning Ship path: i + 1 - log2(log2(r2) / log2(bailout)) for an escaped sample, max_iter otherwise.
    At bailout <= 1 the kernel takes the shader's form as written, through the library log:
    nu = i + 1 - log(log(r2) / log(bailout)) / ln 2 -- NaN where the quotient is negative, -inf at bailout == 1."""
    nu = np.full(it.shape, float(max_iter))
    e = it < max_iter
    b = np.float64(np.float32(bailout))
    with np.errstate(all="ignore"):
        if np.float32(bailout) > np.float32(1.0):
            inv = np.float64(1.0) / np.log2(b)
            nu[e] = (it[e] + 1.0) - np.log2(np.log2(r2[e]) * inv)
        else:
            nu[e] = (it[e].astype(np.float64) + 1.0) - np.log(np.log(r2[e]) / np.log(b)) / np.log(np.float64(2.0))
    return nu


def restate(view: dict, W: int, H: int, aa: int = 1, bailout: float = 4.0, rows=None, orbit=None):
    """Every sub-sample of the frame: a list over s of (iter, r2) planes, the rebases and the folded steps"""
    if orbit is None:
        orbit = reference_orbit(view["cx"], view["cy"], view["zoom"], view["max_iter"], bailout)
    out, rebases, folded = [], 0, 0
    for s in range(aa * aa):
        dcx, dcy = sample_dc(W, H, view["zoom"], aa, s, rows)
        it, r2, rb, fo = perturb(orbit, dcx, dcy, view["max_iter"], bailout)
        out.append((it, r2))
        rebases += rb
        folded += fo
    return out, rebases, folded


def exact_iter(cx: str, cy: str, x: int, y: int, W: int, H: int, zoom: float, max_iter: int, bailout: float = 4.0,
               aa: int = 1, s: int = 0, F: int = 0) -> int:
    """The escape index of one sample by the direct iteration of (|x| + i|y|)^2 + c in fixed point at F + 64 fraction
    bits, c = centre + dc exactly (then rounded once)"""
    G = (F or R.frac_bits(zoom)) + 64
    dcx, dcy = sample_dc(W, H, zoom, aa, s, rows=[y])
    cr = round((Fraction(cx) + Fraction(float(dcx[0, x]))) * (1 << G))
    ci = round((Fraction(cy) + Fraction(float(dcy[0, x]))) * (1 << G))
    b2 = float(np.float32(bailout)) ** 2
    T = Fraction(b2) * (1 << (2 * G))
    zr = zi = 0
    for i in range(max_iter):
        zr, zi = ((zr * zr - zi * zi) >> G) + cr, ((2 * abs(zr) * abs(zi)) >> G) + ci
        if zr * zr + zi * zi > T:
            return i
    return max_iter
