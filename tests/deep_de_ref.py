"""Distance estimates for deep Mandelbrot views (fr_render_deep_de): the header's arithmetic restated operation for operation
in fp64 numpy, and the ground truth in Python integers.

- perturb_de: the per-sample step of deep_bla_ref.perturb_bla (an empty table: deep_ref.perturb's plain step) with the scaled
  derivative D = dz/dc * s carried next to the delta; returns (iter, r2, Dx, Dy, counts);
- de_of: (r2, D) of the escaping update -> the distance estimate in pixel spacings, 0 for interior;
- shade: the debug shader's distance shading of a linear colour, in fp32;
- restate_de: every sub-sample of a frame (or of its rows), s from the whole frame;
- exact_de: the direct iteration of z^2 + c and d <- 2 z d + 1 of one sample in fixed point at F + 64 fraction bits.

deep_ref.py supplies the reference orbit and the sample offsets, deep_bla_ref.py the table; neither is modified.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import deep_bla_ref as BR
import deep_ref as R

# the tip of the antenna at the bottom of fr_render_deep's range: s = zoom / H ~ 1e-292
TIP = dict(cx="-2", cy="0", zoom=1e-290, max_iter=700)


def spacing(zoom: float, H: int) -> np.float64:
    """s = zoom / H of the WHOLE frame: one pixel spacing"""
    return np.float64(zoom) / np.float64(H)


def perturb_de(orbit: np.ndarray, dcx: np.ndarray, dcy: np.ndarray, max_iter: int, table, s, bailout: float = 4.0):
    """perturb_bla with D: D' = 2 z D + s in a plain step (z = Z_m + dz, before the update), D' = A D + B s in a BLA step, a
    rebase leaves it alone.  table == []: no BLA step is ever taken (the plain path).  Returns (iter, r2, Dx, Dy, counts): D of
    the escaping update for an escaped sample, whatever the loop left for the others (de_of never reads it)."""
    ox, oy = np.ascontiguousarray(orbit[:, 0]), np.ascontiguousarray(orbit[:, 1])
    N = len(orbit) - 1
    K = len(table)
    B2 = np.float64(np.float32(bailout)) * np.float64(np.float32(bailout))
    s = np.float64(s)
    shape = dcx.shape
    cx, cy = dcx.ravel().astype(np.float64), dcy.ravel().astype(np.float64)
    n = cx.size
    it = np.full(n, max_iter, np.int32)
    r2out = np.zeros(n, np.float64)
    Dxo = np.zeros(n, np.float64); Dyo = np.zeros(n, np.float64)
    idx = np.arange(n)
    dzx = np.zeros(n); dzy = np.zeros(n)
    Dx = np.zeros(n); Dy = np.zeros(n)
    m = np.zeros(n, np.int64)
    u = np.zeros(n, np.int64)
    counts = [0, 0, 0]
    with np.errstate(all="ignore"):
        while idx.size:
            Zx, Zy = ox[m], oy[m]
            dz2 = dzx * dzx + dzy * dzy
            k = np.zeros(idx.size, np.int64)
            if K:
                r0 = np.float64(BR.EPS) * BR._abs(Zx, Zy)
                cand = np.nonzero((m >= 1) & (dz2 < r0 * r0))[0]
                if cand.size:
                    mc = m[cand]
                    kk = np.minimum(BR._ctz(mc - 1, K), K)
                    kk = np.minimum(kk, BR._flog2(N - mc))
                    kk = np.minimum(kk, BR._flog2(max_iter - u[cand]))
                    for lvl in range(K, 0, -1):
                        sel = np.nonzero(kk == lvl)[0]
                        if sel.size == 0:
                            continue
                        r = table[lvl - 1]["r"][(mc[sel] - 1) >> lvl]
                        bad = ~(dz2[cand[sel]] < r * r)
                        kk[sel[bad]] -= 1
                    k[cand] = np.maximum(kk, 0)
            bl = k > 0
            # the plain step and its derivative, from the point before the update
            zbx = Zx + dzx
            zby = Zy + dzy
            wx = zbx + zbx
            wy = zby + zby
            nDx = (wx * Dx - wy * Dy) + s
            nDy = wx * Dy + wy * Dx
            tx = (Zx + Zx) + dzx
            ty = (Zy + Zy) + dzy
            nx = (tx * dzx - ty * dzy) + cx
            ny = (tx * dzy + ty * dzx) + cy
            if bl.any():
                b = np.nonzero(bl)[0]
                kb = k[b]
                j = (m[b] - 1) >> kb
                ax = np.empty(b.size); ay = np.empty(b.size); bx = np.empty(b.size); by = np.empty(b.size)
                for lvl in np.unique(kb):
                    q = kb == lvl
                    T = table[lvl - 1]
                    ax[q], ay[q], bx[q], by[q] = T["ax"][j[q]], T["ay"][j[q]], T["bx"][j[q]], T["by"][j[q]]
                ex, ey, gx, gy = dzx[b], dzy[b], cx[b], cy[b]
                nx[b] = (ax * ex - ay * ey) + (bx * gx - by * gy)
                ny[b] = (ax * ey + ay * ex) + (bx * gy + by * gx)
                fx, fy = Dx[b], Dy[b]
                nDx[b] = (ax * fx - ay * fy) + bx * s
                nDy[b] = (ax * fy + ay * fx) + by * s
            Dx, Dy = nDx, nDy
            step = np.where(bl, np.left_shift(1, k), 1)
            counts[0] += int((~bl).sum())
            counts[1] += int(bl.sum())
            counts[2] += int(step[bl].sum())
            m = m + step
            u = u + step
            zx = ox[m] + nx
            zy = oy[m] + ny
            r2 = zx * zx + zy * zy
            esc = r2 > B2
            reb = ~esc & ((r2 < nx * nx + ny * ny) | (m == N))
            dzx = np.where(reb, zx, nx)
            dzy = np.where(reb, zy, ny)
            m = np.where(reb, 0, m)
            it[idx[esc]] = (u[esc] - 1).astype(np.int32)
            r2out[idx[esc]] = r2[esc]
            Dxo[idx[esc]] = Dx[esc]
            Dyo[idx[esc]] = Dy[esc]
            keep = ~esc & (u < max_iter)
            if not keep.all():
                idx, dzx, dzy, m, u, cx, cy, Dx, Dy = (a[keep] for a in (idx, dzx, dzy, m, u, cx, cy, Dx, Dy))
    return it.reshape(shape), r2out.reshape(shape), Dxo.reshape(shape), Dyo.reshape(shape), counts


def de_of(it: np.ndarray, r2: np.ndarray, Dx: np.ndarray, Dy: np.ndarray, max_iter: int) -> np.ndarray:
    """zl = sqrt(r2); dl = sqrt(D.x D.x + D.y D.y); de = (zl * log(zl)) / dl; NaN -> 0; interior: 0"""
    e = it < max_iter
    out = np.zeros(it.shape, np.float64)
    with np.errstate(all="ignore"):
        zl = np.sqrt(r2[e])
        dl = np.sqrt(Dx[e] * Dx[e] + Dy[e] * Dy[e])
        de = (zl * np.log(zl)) / dl
    out[e] = np.where(np.isnan(de), 0.0, de)
    return out


def deriv_of(it: np.ndarray, Dx: np.ndarray, Dy: np.ndarray, max_iter: int) -> np.ndarray:
    """the deriv plane: (D.x, D.y) for an escaped sample, (0, 0) for interior"""
    e = it < max_iter
    return np.stack([np.where(e, Dx, 0.0), np.where(e, Dy, 0.0)], axis=-1)


def shade(rgb: np.ndarray, de: np.ndarray, escaped: np.ndarray, edge_px: float) -> np.ndarray:
    """mandelbrot_debug.comp:196-197 with the edge in pixel spacings, fp32, on the escaped samples of a (..., 3) colour"""
    f = np.float32
    with np.errstate(all="ignore"):
        x = de.astype(np.float32) / f(edge_px)
    x = np.minimum(np.maximum(x, f(0.0)), f(1.0))
    sm = x * x * (f(3.0) - f(2.0) * x)
    t = ((f(1.0) - sm) * f(0.3))[..., None]
    rgb = rgb.astype(np.float32)
    out = rgb * (f(1.0) - t) + (rgb * f(0.7)) * t
    return np.where(escaped[..., None], out, rgb).astype(np.float32)


def restate_de(view: dict, W: int, H: int, aa: int = 1, bailout: float = 4.0, rows=None, orbit=None, bla: bool = False):
    """Every sub-sample of the frame (or of its rows): a list over s of (iter, r2, Dx, Dy), and the three counts summed.  s and
    dcmax are those of the whole W x H frame, whatever the rows."""
    if orbit is None:
        orbit = R.reference_orbit(view["cx"], view["cy"], view["zoom"], view["max_iter"], bailout)
    table = BR.bla_table(orbit, BR.dcmax(W, H, view["zoom"])) if bla else []
    sp = spacing(view["zoom"], H)
    out, total = [], [0, 0, 0]
    for q in range(aa * aa):
        dcx, dcy = R.sample_dc(W, H, view["zoom"], aa, q, rows)
        it, r2, Dx, Dy, c = perturb_de(orbit, dcx, dcy, view["max_iter"], table, sp, bailout)
        out.append((it, r2, Dx, Dy))
        total = [a + b for a, b in zip(total, c)]
    return out, total


def exact_de(cx: str, cy: str, x: int, y: int, W: int, H: int, zoom: float, max_iter: int, bailout: float = 4.0, F: int = 0):
    """(iter, de) of one pixel's sample (0,0) by the direct iteration of z <- z^2 + c, d <- 2 z d + 1 (d_0 = 0) in fixed point at
    F + 64 fraction bits, c = centre + dc exactly (then rounded once); de = |z| log|z| / (|d| s) in pixel spacings, 0 for
    interior.  |d| reaches 1 / zoom and more: it stays a Python integer until the last division."""
    G = (F or R.frac_bits(zoom)) + 64
    dcx, dcy = R.sample_dc(W, H, zoom, 1, 0, rows=[y])
    cr = round((Fraction(cx) + Fraction(float(dcx[0, x]))) * (1 << G))
    ci = round((Fraction(cy) + Fraction(float(dcy[0, x]))) * (1 << G))
    b2 = float(np.float32(bailout)) ** 2
    T = Fraction(b2) * (1 << (2 * G))
    one = 1 << G
    zr = zi = dr = di = 0
    for i in range(max_iter):
        dr, di = ((2 * (zr * dr - zi * di)) >> G) + one, (2 * (zr * di + zi * dr)) >> G
        zr, zi = ((zr * zr - zi * zi) >> G) + cr, ((2 * zr * zi) >> G) + ci
        n2 = zr * zr + zi * zi
        if n2 > T:
            zl = math.sqrt(float(Fraction(n2, 1 << (2 * G))))
            dl = Fraction(math.isqrt(dr * dr + di * di), one) * Fraction(float(spacing(zoom, H)))
            return i, float(Fraction(zl * math.log(zl)) / dl)
    return max_iter, 0.0
