"""Distance estimates for deep Julia views (fr_render_deep_julia_de, fr_render_deepx_julia_de): the header's arithmetic restated
operation for operation in numpy, and the ground truth in Python integers.  Built on deep_julia_ref (orbits, sample offsets),
deep_julia_bla_ref (tables, level logic, PRECRIT60) and deepx_de_ref / deep_de_ref (the two planes, the shading); none of them is
modified.

- perturb_de: deep_julia_bla_ref.perturb_bla with the scaled derivative D = dz_n/dz_0 * s next to the delta; with the empty pair
  of tables no BLA step is ever taken and it is deep_julia_ref.perturb's loop;
- perturb_x_de: deep_julia_bla_ref.perturb_x_bla with D an extended complex number (Dx, Dy, eD), normalised and flushed after
  every update; stats receives the smallest and largest exponent sum of a D update, the smallest exponent of a D before its
  flush, and the flushes;
- restate_de / restate_x_de: every sub-sample of a frame (or of its rows);
- exact_de / exact_de_x: the direct iteration of z <- z^2 + c and G <- 2 z G (G_0 = 1) of one sample in fixed point at F + 64
  fraction bits; de = |z| log|z| / (|G| s) in pixel spacings;
- the view PRECRIT200 of the extended entry point.
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

import deep_bla_ref as BR
import deep_de_ref as DE
import deep_julia_bla_ref as JB
import deep_julia_ref as J
import deep_ship_ref as S
import deepx_de_ref as XD
import deepx_ref as X
from deepx_ref import X_THR, X_ZERO, _ld, _norm

EPS = BR.EPS
X_FLUSH = J.X_FLUSH              # a normalised D with e below this becomes the zero, as a delta does
NO_TABLES = ([], [])
shade = DE.shade
de_of, deriv_of = DE.de_of, DE.deriv_of
de_of_x, deriv_of_x = XD.de_of_x, XD.deriv_of_x
spacing, spacing_x = DE.spacing, XD.spacing_x


# ---- fp64 ------------------------------------------------------------------------------------------------------------------
def perturb_de(P: np.ndarray, Q: np.ndarray, tabs, d0x: np.ndarray, d0y: np.ndarray, max_iter: int, s, bailout: float = 4.0):
    """Returns (iter, r2, Dx, Dy, counts): D of the escaping update for an escaped sample, zeros for the others (de_of never
    reads them); counts = [plain steps, BLA steps, updates skipped]."""
    ox = np.concatenate([Q[:, 0], P[:, 0]])
    oy = np.concatenate([Q[:, 1], P[:, 1]])
    NQ, NP, poff = len(Q) - 1, len(P) - 1, len(Q)
    KQ, KP = len(tabs[0]), len(tabs[1])
    T = JB._joined(tabs, ("r", "ax", "ay"))
    B2 = np.float64(np.float32(bailout)) * np.float64(np.float32(bailout))
    shape = d0x.shape
    dzx, dzy = d0x.ravel().astype(np.float64).copy(), d0y.ravel().astype(np.float64).copy()
    n = dzx.size
    it = np.full(n, max_iter, np.int32)
    r2out = np.zeros(n, np.float64)
    Dxo = np.zeros(n); Dyo = np.zeros(n)
    idx = np.arange(n)
    m = np.zeros(n, np.int64)
    u = np.zeros(n, np.int64)
    onp = np.ones(n, bool)
    Dx = np.full(n, np.float64(s)); Dy = np.zeros(n)               # D = (s, +0.0)
    counts = [0, 0, 0]
    with np.errstate(all="ignore"):
        while idx.size:
            base = np.where(onp, poff, 0)
            N = np.where(onp, NP, NQ)
            Kl = np.where(onp, KP, KQ)
            Zx, Zy = ox[base + m], oy[base + m]
            dz2 = dzx * dzx + dzy * dzy
            k = np.zeros(idx.size, np.int64)
            r0 = np.float64(EPS) * BR._abs(Zx, Zy)
            cand = np.nonzero((m >= 1) & (dz2 < r0 * r0) & (Kl > 0))[0]
            if cand.size:
                mc, pc = m[cand], onp[cand]
                kk = JB._top_level(mc, Kl[cand], N[cand], max_iter, u[cand])
                for lvl in range(len(T), 0, -1):
                    sel = np.nonzero(kk == lvl)[0]
                    if sel.size == 0:
                        continue
                    r = T[lvl - 1]["r"][((mc[sel] - 1) >> lvl) + np.where(pc[sel], T[lvl - 1]["off"], 0)]
                    bad = ~(dz2[cand[sel]] < r * r)
                    kk[sel[bad]] -= 1
                k[cand] = np.maximum(kk, 0)
            bl = k > 0
            # the plain step and its derivative, from the point before the update: z = Z_m + dz, w = z + z, D' = w D
            zbx = Zx + dzx
            zby = Zy + dzy
            wx = zbx + zbx
            wy = zby + zby
            nDx = wx * Dx - wy * Dy
            nDy = wx * Dy + wy * Dx
            tx = (Zx + Zx) + dzx
            ty = (Zy + Zy) + dzy
            nx = tx * dzx - ty * dzy
            ny = tx * dzy + ty * dzx
            if bl.any():
                b = np.nonzero(bl)[0]
                kb = k[b]
                ax = np.empty(b.size); ay = np.empty(b.size)
                for lvl in np.unique(kb):
                    q = kb == lvl
                    j = ((m[b[q]] - 1) >> lvl) + np.where(onp[b[q]], T[lvl - 1]["off"], 0)
                    ax[q], ay[q] = T[lvl - 1]["ax"][j], T[lvl - 1]["ay"][j]
                ex, ey = dzx[b], dzy[b]
                nx[b] = ax * ex - ay * ey
                ny[b] = ax * ey + ay * ex
                fx, fy = Dx[b], Dy[b]
                nDx[b] = ax * fx - ay * fy                          # D' = A D
                nDy[b] = ax * fy + ay * fx
            Dx, Dy = nDx, nDy
            step = np.where(bl, np.left_shift(1, k), 1)
            counts[0] += int((~bl).sum())
            counts[1] += int(bl.sum())
            counts[2] += int(step[bl].sum())
            m = m + step
            u = u + step
            zx = ox[base + m] + nx
            zy = oy[base + m] + ny
            r2 = zx * zx + zy * zy
            esc = r2 > B2
            reb = ~esc & ((r2 < nx * nx + ny * ny) | (m == N))
            dzx = np.where(reb, zx, nx)
            dzy = np.where(reb, zy, ny)
            m = np.where(reb, 0, m)
            onp = onp & ~reb
            it[idx[esc]] = (u[esc] - 1).astype(np.int32)
            r2out[idx[esc]] = r2[esc]
            Dxo[idx[esc]], Dyo[idx[esc]] = Dx[esc], Dy[esc]
            keep = ~esc & (u < max_iter)
            if not keep.all():
                idx, dzx, dzy, m, u, onp, Dx, Dy = (a[keep] for a in (idx, dzx, dzy, m, u, onp, Dx, Dy))
    return it.reshape(shape), r2out.reshape(shape), Dxo.reshape(shape), Dyo.reshape(shape), counts


def restate_de(v: dict, W: int, H: int, aa: int = 1, bailout: float = 4.0, rows=None, orbits=None, bla: bool = False, tabs=None):
    """Every sub-sample of the frame (or of its rows): a list over s of (iter, r2, Dx, Dy), and the three counts summed.  s is
    that of the whole W x H frame, whatever the rows."""
    P, Q = orbits if orbits is not None else J.reference_orbits(v, bailout)
    if not bla:
        tabs = NO_TABLES
    elif tabs is None:
        tabs = JB.bla_tables(P, Q)
    sp = spacing(v["zoom"], H)
    out, total = [], [0, 0, 0]
    for q in range(aa * aa):
        d0x, d0y = S.sample_dc(W, H, v["zoom"], aa, q, rows)
        it, r2, Dx, Dy, c = perturb_de(P, Q, tabs, d0x, d0y, v["max_iter"], sp, bailout)
        out.append((it, r2, Dx, Dy))
        total = [a + b for a, b in zip(total, c)]
    return out, total


# ---- extended --------------------------------------------------------------------------------------------------------------
def _note(stats, eP, eN, fl):
    """what a D update did: its exponent sum, the exponent of the normalised result in front of the flush, the flushes"""
    if stats is None or eP.size == 0:
        return
    stats["sum_min"] = min(stats.get("sum_min", 0), int(eP.min()))
    stats["sum_max"] = max(stats.get("sum_max", 0), int(eP.max()))
    live = eN != X_ZERO
    if live.any():
        stats["e_min"] = min(stats.get("e_min", 0), int(eN[live].min()))
        stats["e_max"] = max(stats.get("e_max", -(1 << 40)), int(eN[live].max()))
    stats["d_flushes"] = stats.get("d_flushes", 0) + int((fl & live).sum())


def _d_set(px, py, ep, stats=None):
    """D' = norm(p), then the flush"""
    x, y, e = _norm(px, py, ep)
    fl = e < X_FLUSH
    _note(stats, np.asarray(ep), e, fl)
    return np.where(fl, 0.0, x), np.where(fl, 0.0, y), np.where(fl, X_ZERO, e)


def perturb_x_de(Px, Qx, tabs, d0, max_iter: int, s, bailout: float = 4.0, stats=None):
    """Returns (iter, r2, Dx, Dy, eD, counts)"""
    mant = np.concatenate([Qx[0], Px[0]])
    exp2 = np.concatenate([Qx[1], Px[1]])
    omx, omy = np.ascontiguousarray(mant[:, 0]), np.ascontiguousarray(mant[:, 1])
    oe = exp2.astype(np.int64)
    plain = X.decode(mant, exp2)
    opx, opy = np.ascontiguousarray(plain[:, 0]), np.ascontiguousarray(plain[:, 1])
    NQ, NP, poff = len(Qx[1]) - 1, len(Px[1]) - 1, len(Qx[1])
    KQ, KP = len(tabs[0]), len(tabs[1])
    T = JB._joined(tabs, ("rv", "re", "ax", "ay", "ea"))
    B2 = np.float64(np.float32(bailout)) * np.float64(np.float32(bailout))
    x0, y0, e0 = d0
    n = x0.size
    it = np.full(n, max_iter, np.int32)
    r2out = np.zeros(n, np.float64)
    Dxo = np.zeros(n); Dyo = np.zeros(n)
    eDo = np.full(n, X_ZERO, np.int64)
    idx = np.arange(n)
    ext = e0 <= X_THR
    with np.errstate(all="ignore"):
        dx = np.where(ext, x0, _ld(x0, np.where(ext, 0, e0)))
        dy = np.where(ext, y0, _ld(y0, np.where(ext, 0, e0)))
    ed = e0.astype(np.int64).copy()
    m = np.zeros(n, np.int64)
    u = np.zeros(n, np.int64)
    onp = np.ones(n, bool)
    Dx = np.full(n, np.float64(s[0])); Dy = np.zeros(n)            # D = (sm, +0.0, es)
    eD = np.full(n, np.int64(s[1]), np.int64)
    counts = [0, 0, 0]

    def finish(Sx, bb, NN, mm, nx, ny, en, esc, r2e):
        Wx, Wy, eW = omx[bb + mm], omy[bb + mm], oe[bb + mm]
        ez = np.maximum(eW, en)
        zx = _ld(Wx, eW - ez) + _ld(nx, en - ez)
        zy = _ld(Wy, eW - ez) + _ld(ny, en - ez)
        r2 = zx * zx + zy * zy
        r2d = _ld(r2, 2 * ez)
        es = r2d > B2
        n2 = nx * nx + ny * ny
        reb = ~es & ((r2 < _ld(n2, 2 * (en - ez))) | (mm == NN))
        ax, ay, ea = _norm(np.where(reb, zx, nx), np.where(reb, zy, ny), np.where(reb, ez, en))
        fl = ea < X_FLUSH
        ax, ay, ea = np.where(fl, 0.0, ax), np.where(fl, 0.0, ay), np.where(fl, X_ZERO, ea)
        stay = ea <= X_THR
        dx[Sx] = np.where(stay, ax, _ld(ax, np.where(stay, 0, ea)))
        dy[Sx] = np.where(stay, ay, _ld(ay, np.where(stay, 0, ea)))
        ed[Sx] = ea
        ext[Sx] = stay
        m[Sx] = np.where(reb, 0, mm)
        onp[Sx] = onp[Sx] & ~reb
        esc[Sx] = es
        r2e[Sx] = r2d

    with np.errstate(all="ignore"):
        while idx.size:
            base = np.where(onp, poff, 0)
            N = np.where(onp, NP, NQ)
            Kl = np.where(onp, KP, KQ)
            esc = np.zeros(idx.size, bool)
            r2e = np.zeros(idx.size)
            k = np.zeros(idx.size, np.int64)
            cand = np.nonzero((m >= 1) & (Kl > 0))[0]
            if cand.size:
                qx, qy, qe = _norm(dx[cand], dy[cand], np.zeros(cand.size, np.int64))
                isx = ext[cand]
                qx, qy, qe = np.where(isx, dx[cand], qx), np.where(isx, dy[cand], qy), np.where(isx, ed[cand], qe)
                dz2 = qx * qx + qy * qy
                mc, pc = m[cand], onp[cand]
                kk = JB._top_level(mc, Kl[cand], N[cand], max_iter, u[cand])
                for lvl in range(len(T), 0, -1):
                    sel = np.nonzero(kk == lvl)[0]
                    if sel.size == 0:
                        continue
                    j = ((mc[sel] - 1) >> lvl) + np.where(pc[sel], T[lvl - 1]["off"], 0)
                    rv, re = T[lvl - 1]["rv"][j], T[lvl - 1]["re"][j]
                    bad = ~(dz2[sel] < _ld(rv * rv, 2 * (re - qe[sel])))
                    kk[sel[bad]] -= 1
                kk = np.maximum(kk, 0)
                k[cand] = kk
                b = np.nonzero(kk > 0)[0]
                if b.size:
                    Bl = cand[b]
                    kb = kk[b]
                    ax = np.empty(b.size); ay = np.empty(b.size); ea = np.empty(b.size, np.int64)
                    for lvl in np.unique(kb):
                        q = kb == lvl
                        j = ((mc[b[q]] - 1) >> lvl) + np.where(pc[b[q]], T[lvl - 1]["off"], 0)
                        ax[q], ay[q], ea[q] = T[lvl - 1]["ax"][j], T[lvl - 1]["ay"][j], T[lvl - 1]["ea"][j]
                    fx, fy, fe = Dx[Bl], Dy[Bl], eD[Bl]             # D' = norm(A (x) D, A.e + D.e)
                    Dx[Bl], Dy[Bl], eD[Bl] = _d_set(ax * fx - ay * fy, ax * fy + ay * fx, ea + fe, stats)
                    x, y, e = qx[b], qy[b], qe[b]
                    finish(Bl, base[Bl], N[Bl], mc[b] + np.left_shift(1, kb), ax * x - ay * y, ax * y + ay * x, ea + e, esc, r2e)
            bl = k > 0
            E = np.nonzero(ext & ~bl)[0]
            Pl = np.nonzero(~ext & ~bl)[0]
            if E.size:
                mm, bb = m[E], base[E]
                Zx, Zy, eZ = omx[bb + mm], omy[bb + mm], oe[bb + mm]
                x, y, e = dx[E], dy[E], ed[E]
                ebm = np.maximum(eZ, e)                             # b = Z_m (+) dz, P = b D at eb + 1 + D.e
                bx = _ld(Zx, eZ - ebm) + _ld(x, e - ebm)
                by = _ld(Zy, eZ - ebm) + _ld(y, e - ebm)
                fx, fy, fe = Dx[E], Dy[E], eD[E]
                Dx[E], Dy[E], eD[E] = _d_set(bx * fx - by * fy, bx * fy + by * fx, ebm + 1 + fe, stats)
                et = np.maximum(eZ + 1, e)
                tx = _ld(Zx, eZ + 1 - et) + _ld(x, e - et)
                ty = _ld(Zy, eZ + 1 - et) + _ld(y, e - et)
                finish(E, bb, N[E], mm + 1, tx * x - ty * y, tx * y + ty * x, et + e, esc, r2e)
            if Pl.size:
                mm, bb = m[Pl], base[Pl]
                Zx, Zy = opx[bb + mm], opy[bb + mm]
                x, y = dx[Pl], dy[Pl]
                zbx = Zx + x                                        # w = 2 (Z_m + dz) on the plain doubles, P = w D at D.e
                zby = Zy + y
                wx = zbx + zbx
                wy = zby + zby
                fx, fy, fe = Dx[Pl], Dy[Pl], eD[Pl]
                Dx[Pl], Dy[Pl], eD[Pl] = _d_set(wx * fx - wy * fy, wx * fy + wy * fx, fe, stats)
                tx = (Zx + Zx) + x
                ty = (Zy + Zy) + y
                nx = tx * x - ty * y
                ny = tx * y + ty * x
                mm = mm + 1
                zx = opx[bb + mm] + nx
                zy = opy[bb + mm] + ny
                r2 = zx * zx + zy * zy
                es = r2 > B2
                reb = ~es & ((r2 < nx * nx + ny * ny) | (mm == N[Pl]))
                ax = np.where(reb, zx, nx)
                ay = np.where(reb, zy, ny)
                small = np.maximum(np.abs(ax), np.abs(ay)) < X._THR
                bx, by, be = _norm(ax, ay, np.zeros(Pl.size, np.int64))
                dx[Pl] = np.where(small, bx, ax)
                dy[Pl] = np.where(small, by, ay)
                ed[Pl] = be
                ext[Pl] = small
                m[Pl] = np.where(reb, 0, mm)
                onp[Pl] = onp[Pl] & ~reb
                esc[Pl] = es
                r2e[Pl] = r2
            step = np.where(bl, np.left_shift(1, k), 1)
            counts[0] += int((~bl).sum())
            counts[1] += int(bl.sum())
            counts[2] += int(step[bl].sum())
            u = u + step
            it[idx[esc]] = (u[esc] - 1).astype(np.int32)
            r2out[idx[esc]] = r2e[esc]
            Dxo[idx[esc]], Dyo[idx[esc]], eDo[idx[esc]] = Dx[esc], Dy[esc], eD[esc]
            keep = ~esc & (u < max_iter)
            if not keep.all():
                idx, dx, dy, ed, ext, m, u, onp, Dx, Dy, eD = (a[keep] for a in (idx, dx, dy, ed, ext, m, u, onp, Dx, Dy, eD))
    return it, r2out, Dxo, Dyo, eDo, counts


def restate_x_de(v: dict, W: int, H: int, aa: int = 1, bailout: float = 4.0, rows=None, orbits=None, bla: bool = False, tabs=None,
                 stats=None):
    """Every sub-sample of the frame (or of its rows) through the extended restatement (the view's zoom_s): a list over s of
    (iter, r2, Dx, Dy, eD) planes, and the three counts summed"""
    Px, Qx = orbits if orbits is not None else J.reference_orbits_x(v, bailout)
    if not bla:
        tabs = NO_TABLES
    elif tabs is None:
        tabs = JB.bla_tables_x(Px, Qx)
    zm, ze = X.zoom_pair(v["zoom_s"])
    sp = spacing_x(zm, ze, H)
    nrows = H if rows is None else len(rows)
    out, total = [], [0, 0, 0]
    for q in range(aa * aa):
        r = perturb_x_de(Px, Qx, tabs, J.sample_d0_x(W, H, zm, ze, aa, q, rows), v["max_iter"], sp, bailout, stats)
        out.append(tuple(a.reshape(nrows, W) for a in r[:5]))
        total = [a + b for a, b in zip(total, r[5])]
    return out, total


# ---- the exact derivative ----------------------------------------------------------------------------------------------------
def _exact_de(v: dict, z0r: Fraction, z0i: Fraction, sp: Fraction, bailout: float):
    """(iter, de): z <- z^2 + c and G <- 2 z G, G_0 = 1, in Python ints at F + 64 fraction bits, G updated from the point before
    the update; de = |z| log|z| / (|G| s), 0 for interior.  |G| reaches 1 / zoom and more: it stays an integer until the last
    division."""
    Gb = v["F"] + 64
    zr, zi = round(z0r * (1 << Gb)), round(z0i * (1 << Gb))
    cr, ci = J.c_fixed(v["c"][0], Gb), J.c_fixed(v["c"][1], Gb)
    T = int(Fraction(float(np.float32(bailout)) ** 2) * (1 << (2 * Gb)))
    one = 1 << Gb
    gr, gi = one, 0
    for i in range(v["max_iter"]):
        gr, gi = (2 * (zr * gr - zi * gi)) >> Gb, (2 * (zr * gi + zi * gr)) >> Gb
        zr, zi = ((zr * zr - zi * zi) >> Gb) + cr, ((2 * zr * zi) >> Gb) + ci
        n2 = zr * zr + zi * zi
        if n2 > T:
            zl = math.sqrt(float(Fraction(n2, 1 << (2 * Gb))))
            dl = Fraction(math.isqrt(gr * gr + gi * gi), one) * sp
            return i, (float(Fraction(zl * math.log(zl)) / dl) if dl else math.inf)
    return v["max_iter"], 0.0


def exact_de(v: dict, x: int, y: int, W: int, H: int, bailout: float = 4.0):
    """of sample (0,0) of pixel (x, y) of the fp64 entry point: d0 the kernel's double, s = the double zoom / H, both exact"""
    d0x, d0y = S.sample_dc(W, H, v["zoom"], 1, 0, rows=[y])
    return _exact_de(v, Fraction(v["cx"]) + Fraction(float(d0x[0, x])), Fraction(v["cy"]) + Fraction(float(d0y[0, x])),
                     Fraction(float(spacing(v["zoom"], H))), bailout)


def exact_de_x(v: dict, x: int, y: int, W: int, H: int, bailout: float = 4.0):
    """of the extended entry point: d0 = (mantissas formed with zm) 2^ze, s = sm 2^es, exact"""
    zm, ze = X.zoom_pair(v["zoom_s"])
    mx, my = S.sample_dc(W, H, zm, 1, 0, rows=[y])
    z2 = Fraction(2) ** ze
    sm, es = spacing_x(zm, ze, H)
    return _exact_de(v, Fraction(v["cx"]) + Fraction(float(mx[0, x])) * z2, Fraction(v["cy"]) + Fraction(float(my[0, x])) * z2,
                     Fraction(float(sm)) * Fraction(2) ** es, bailout)


# ---- views ---------------------------------------------------------------------------------------------------------------------
PRECRIT200_ITER = 1200         # 300 .. 1000: no sample escapes; 1100 .. 1700: 767 of the 768 pixels of a 32 x 24 frame, iter 1049 .. 1069


@functools.lru_cache(maxsize=None)
def _precrit200():
    cx, cy = JB.precritical_centre((0.0, 1.0), 12, 201)
    return dict(name="PRECRIT200", c=(0.0, 1.0), cx=cx, cy=cy, zoom=1e-200, zoom_s="1e-200", max_iter=PRECRIT200_ITER,
                F=X.frac_bits_x("1e-200"))


def view(name: str) -> dict:
    """deep_julia_bla_ref's views and PRECRIT200 (extended entry point only): the dendrite at 1e-200 around a depth-12 preimage
    of 0 quantised to 201 decimals.  P_12 is of the size of the deltas, so |2 z| of that update is about 1e-200 and D's exponent
    drops by about 650 in one update and climbs back.  max_iter was chosen on the CPU with the extended restatement so that at
    least 90 % of the 32 x 24 pixels escape (test_deep_julia_de_host.py asserts it)."""
    return _precrit200() if name == "PRECRIT200" else JB.view(name)


def basin_view(c, max_iter: int = 64) -> dict:
    """a superattracting basin in the extended loop (c = 0, c = -1): centre 0.25 at zoom 0.5, so that every sample runs to the
    critical orbit's cycle, its |2 z| squaring itself towards nothing -- the flush of D"""
    return dict(name="basin", c=c, cx="0.25", cy="0", zoom=0.5, zoom_s="0.5", max_iter=max_iter, F=X.frac_bits_x("0.5"))


# ---- what the tests share: computed once per session, never changed ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def orbits(name: str):
    return J.reference_orbits(view(name))


@functools.lru_cache(maxsize=None)
def orbits_x(name: str):
    return J.reference_orbits_x(view(name))


@functools.lru_cache(maxsize=None)
def restated(name: str, W: int, H: int, aa: int = 1, bla: bool = False):
    return restate_de(view(name), W, H, aa, orbits=orbits(name), bla=bla)


@functools.lru_cache(maxsize=None)
def restated_x(name: str, W: int, H: int, aa: int = 1, bla: bool = False):
    return restate_x_de(view(name), W, H, aa, orbits=orbits_x(name), bla=bla)


def sampled(W: int = 48, H: int = 36, every: int = 53):
    """every 53rd pixel of a frame: (ys, xs)"""
    k = np.arange(0, W * H, every)
    return k // W, k % W
