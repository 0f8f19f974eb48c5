"""Distance estimates for extended views (fr_render_deepx_de): the header's arithmetic restated operation for operation in
numpy, and the ground truth in Python integers.

- spacing_x: one pixel spacing s = (sm, es) = norm1(zm / H, ze) of the whole frame;
- perturb_x_de: the two-mode step of deepx_ref.perturb_x -- with a table, of deepx_bla_ref.perturb_x_bla -- with the scaled
  derivative D = dz/dc * s carried as an extended complex number (Dx, Dy, eD); returns (iter, r2, Dx, Dy, eD, counts);
- de_of_x / deriv_of_x: (r2, D) of the escaping update -> the two planes;
- restate_x_de: every sub-sample of a frame (or of its rows), s and dcmax from the whole frame;
- exact_de_x: the direct iteration of z^2 + c and d <- 2 z d + 1 of one sample in fixed point at F + 64 fraction bits.

deepx_ref.py supplies the orbit, the sample offsets and the extended helpers, deepx_bla_ref.py the table and the level logic,
deep_de_ref.py the shading; none of them is modified.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import deep_bla_ref as BR
import deep_de_ref as DE
import deep_ref as R
import deepx_bla_ref as XB
import deepx_ref as X
from deepx_ref import X_THR, X_ZERO, _ld, _norm

shade = DE.shade                                                  # the shading is fr_render_deep_de's, unchanged


def spacing_x(zm: float, ze: int, H: int):
    """(sm, es): zm / (double)H rounded once, then normalised into [0.5, 1)"""
    m, k = math.frexp(float(np.float64(zm) / np.float64(H)))
    return np.float64(m), int(ze) + k


def _d_set(px, py, ep, qx, qy, eq):
    """norm(p (+) q): both aligned on the larger exponent; qy None: q is real and nothing is added to the imaginary part"""
    e = np.maximum(ep, eq)
    x = _ld(px, ep - e) + _ld(qx, eq - e)
    y = _ld(py, ep - e)
    if qy is not None:
        y = y + _ld(qy, eq - e)
    return _norm(x, y, e)


def perturb_x_de(mant, exp2, dc, max_iter: int, table, s, bailout: float = 4.0):
    """perturb_x_bla with D.  table == []: no BLA step is ever taken (deepx_ref.perturb_x's path).  Returns (iter, r2, Dx, Dy,
    eD, counts): D of the escaping update for an escaped sample, zeros for the others (de_of_x never reads them)."""
    omx, omy = np.ascontiguousarray(mant[:, 0]), np.ascontiguousarray(mant[:, 1])
    oe = exp2.astype(np.int64)
    plain = X.decode(mant, exp2)
    opx, opy = np.ascontiguousarray(plain[:, 0]), np.ascontiguousarray(plain[:, 1])
    N = len(oe) - 1
    K = len(table)
    B2 = np.float64(np.float32(bailout)) * np.float64(np.float32(bailout))
    sm, es = np.float64(s[0]), np.int64(s[1])
    cx, cy, ec, cpx, cpy = dc
    n = cx.size
    it = np.full(n, max_iter, np.int32)
    r2out = np.zeros(n, np.float64)
    Dxo = np.zeros(n); Dyo = np.zeros(n)
    eDo = np.full(n, X_ZERO, np.int64)
    idx = np.arange(n)
    dx = np.zeros(n); dy = np.zeros(n)
    ed = np.full(n, X_ZERO, np.int64)
    ext = np.ones(n, bool)
    m = np.zeros(n, np.int64)
    u = np.zeros(n, np.int64)
    Dx = np.zeros(n); Dy = np.zeros(n)
    eD = np.full(n, X_ZERO, np.int64)
    counts = [0, 0, 0]

    def finish(S, mm, nx, ny, en, esc, r2e):
        """z = Z_m (+) n, the escape test, the rebase rule, norm and the mode rule of the EXTENDED step, for the samples S"""
        Wx, Wy, eW = omx[mm], omy[mm], oe[mm]
        ez = np.maximum(eW, en)
        zx = _ld(Wx, eW - ez) + _ld(nx, en - ez)
        zy = _ld(Wy, eW - ez) + _ld(ny, en - ez)
        r2 = zx * zx + zy * zy
        r2d = _ld(r2, 2 * ez)
        esx = r2d > B2
        n2 = nx * nx + ny * ny
        reb = ~esx & ((r2 < _ld(n2, 2 * (en - ez))) | (mm == N))
        ax, ay, ea = _norm(np.where(reb, zx, nx), np.where(reb, zy, ny), np.where(reb, ez, en))
        stay = ea <= X_THR
        dx[S] = np.where(stay, ax, _ld(ax, np.where(stay, 0, ea)))
        dy[S] = np.where(stay, ay, _ld(ay, np.where(stay, 0, ea)))
        ed[S] = ea
        ext[S] = stay
        m[S] = np.where(reb, 0, mm)
        esc[S] = esx
        r2e[S] = r2d

    with np.errstate(all="ignore"):
        while idx.size:
            esc = np.zeros(idx.size, bool)
            r2e = np.zeros(idx.size)
            k = np.zeros(idx.size, np.int64)
            cand = np.nonzero(m >= 1)[0] if K else np.zeros(0, np.int64)
            if cand.size:
                qx, qy, qe = _norm(dx[cand], dy[cand], np.zeros(cand.size, np.int64))
                isx = ext[cand]
                qx, qy, qe = np.where(isx, dx[cand], qx), np.where(isx, dy[cand], qy), np.where(isx, ed[cand], qe)
                dz2 = qx * qx + qy * qy
                mc = m[cand]
                kk = np.minimum(BR._ctz(mc - 1, K), K)
                kk = np.minimum(kk, BR._flog2(N - mc))
                kk = np.minimum(kk, BR._flog2(max_iter - u[cand]))
                for lvl in range(K, 0, -1):                           # top down: the largest valid k
                    sel = np.nonzero(kk == lvl)[0]
                    if sel.size == 0:
                        continue
                    T = table[lvl - 1]
                    j = (mc[sel] - 1) >> lvl
                    rv, re = T["rv"][j], T["re"][j]
                    bad = ~(dz2[sel] < _ld(rv * rv, 2 * (re - qe[sel])))
                    kk[sel[bad]] -= 1
                kk = np.maximum(kk, 0)
                k[cand] = kk
                b = np.nonzero(kk > 0)[0]
                if b.size:
                    Bl = cand[b]
                    kb = kk[b]
                    j = (mc[b] - 1) >> kb
                    ax = np.empty(b.size); ay = np.empty(b.size); bx = np.empty(b.size); by = np.empty(b.size)
                    ea = np.empty(b.size, np.int64); eb = np.empty(b.size, np.int64)
                    for lvl in np.unique(kb):
                        q = kb == lvl
                        T = table[lvl - 1]
                        ax[q], ay[q], ea[q] = T["ax"][j[q]], T["ay"][j[q]], T["ea"][j[q]]
                        bx[q], by[q], eb[q] = T["bx"][j[q]], T["by"][j[q]], T["eb"][j[q]]
                    # D' = norm((A (x) D, A.e + D.e) (+) (B (sm, 0), B.e + es))
                    fx, fy, fe = Dx[Bl], Dy[Bl], eD[Bl]
                    Dx[Bl], Dy[Bl], eD[Bl] = _d_set(ax * fx - ay * fy, ax * fy + ay * fx, ea + fe, bx * sm, by * sm, eb + es)
                    x, y, e = qx[b], qy[b], qe[b]
                    gx, gy, ge = cx[Bl], cy[Bl], ec[Bl]
                    px, py, ep = ax * x - ay * y, ax * y + ay * x, ea + e
                    sx, sy, eq = bx * gx - by * gy, bx * gy + by * gx, eb + ge
                    en = np.maximum(ep, eq)
                    nx = _ld(px, ep - en) + _ld(sx, eq - en)
                    ny = _ld(py, ep - en) + _ld(sy, eq - en)
                    finish(Bl, mc[b] + np.left_shift(1, kb), nx, ny, en, esc, r2e)
            bl = k > 0
            E = np.nonzero(ext & ~bl)[0]
            P = np.nonzero(~ext & ~bl)[0]
            # (a BLA step may have changed ext of its own lanes: E and P are the single-step lanes, excluded by index)
            if E.size:
                mm = m[E]
                Zx, Zy, eZ = omx[mm], omy[mm], oe[mm]
                x, y, e = dx[E], dy[E], ed[E]
                # D' from the point before the update: b = Z_m (+) dz, P = b D at eb + 1 + D.e
                ebm = np.maximum(eZ, e)
                bx = _ld(Zx, eZ - ebm) + _ld(x, e - ebm)
                by = _ld(Zy, eZ - ebm) + _ld(y, e - ebm)
                fx, fy, fe = Dx[E], Dy[E], eD[E]
                Dx[E], Dy[E], eD[E] = _d_set(bx * fx - by * fy, bx * fy + by * fx, ebm + 1 + fe, sm, None, es)
                et = np.maximum(eZ + 1, e)
                tx = _ld(Zx, eZ + 1 - et) + _ld(x, e - et)
                ty = _ld(Zy, eZ + 1 - et) + _ld(y, e - et)
                px = tx * x - ty * y
                py = tx * y + ty * x
                ep = et + e
                en = np.maximum(ep, ec[E])
                nx = _ld(px, ep - en) + _ld(cx[E], ec[E] - en)
                ny = _ld(py, ep - en) + _ld(cy[E], ec[E] - en)
                finish(E, mm + 1, nx, ny, en, esc, r2e)
            if P.size:
                mm = m[P]
                Zx, Zy = opx[mm], opy[mm]
                x, y = dx[P], dy[P]
                # D': w = 2 (Z_m + dz) on the plain doubles, P = w D at D.e
                zbx = Zx + x
                zby = Zy + y
                wx = zbx + zbx
                wy = zby + zby
                fx, fy, fe = Dx[P], Dy[P], eD[P]
                Dx[P], Dy[P], eD[P] = _d_set(wx * fx - wy * fy, wx * fy + wy * fx, fe, sm, None, es)
                tx = (Zx + Zx) + x
                ty = (Zy + Zy) + y
                nx = (tx * x - ty * y) + cpx[P]
                ny = (tx * y + ty * x) + cpy[P]
                mm = mm + 1
                zx = opx[mm] + nx
                zy = opy[mm] + ny
                r2 = zx * zx + zy * zy
                esx = r2 > B2
                reb = ~esx & ((r2 < nx * nx + ny * ny) | (mm == N))
                ax = np.where(reb, zx, nx)
                ay = np.where(reb, zy, ny)
                small = np.maximum(np.abs(ax), np.abs(ay)) < X._THR
                bx, by, be = _norm(ax, ay, np.zeros(P.size, np.int64))
                dx[P] = np.where(small, bx, ax)
                dy[P] = np.where(small, by, ay)
                ed[P] = be
                ext[P] = small
                m[P] = np.where(reb, 0, mm)
                esc[P] = esx
                r2e[P] = r2
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
                idx, dx, dy, ed, ext, m, u = idx[keep], dx[keep], dy[keep], ed[keep], ext[keep], m[keep], u[keep]
                cx, cy, ec, cpx, cpy = cx[keep], cy[keep], ec[keep], cpx[keep], cpy[keep]
                Dx, Dy, eD = Dx[keep], Dy[keep], eD[keep]
    return it, r2out, Dxo, Dyo, eDo, counts


def de_of_x(it, r2, Dx, Dy, eD, max_iter: int) -> np.ndarray:
    """zl = sqrt(r2); dl = sqrt(D.x D.x + D.y D.y) on the mantissas; de = ldexp((zl * log(zl)) / dl, -D.e), a NaN quotient 0;
    interior: 0"""
    e = it < max_iter
    out = np.zeros(it.shape, np.float64)
    with np.errstate(all="ignore"):
        zl = np.sqrt(r2[e])
        dl = np.sqrt(Dx[e] * Dx[e] + Dy[e] * Dy[e])
        q = (zl * np.log(zl)) / dl
        out[e] = _ld(np.where(np.isnan(q), 0.0, q), -eD[e])
    return out


def deriv_of_x(it, Dx, Dy, eD, max_iter: int) -> np.ndarray:
    """the deriv plane: (ldexp(D.x, D.e), ldexp(D.y, D.e)) for an escaped sample, (0, 0) for interior"""
    e = it < max_iter
    with np.errstate(all="ignore"):
        return np.stack([np.where(e, _ld(Dx, eD), 0.0), np.where(e, _ld(Dy, eD), 0.0)], axis=-1)


def restate_x_de(view: dict, W: int, H: int, aa: int = 1, rows=None, bla: bool = False, bailout: float = 4.0, orbit=None,
                 table=None):
    """Every sub-sample of the frame (or of its rows): a list over s of (iter, r2, Dx, Dy, eD) planes, and the three counts
    summed.  s and dcmax are those of the whole W x H frame, whatever the rows."""
    mant, exp2 = orbit if orbit is not None else X.orbit_of(view, bailout)
    zm, ze = X.zoom_pair(view["zoom"])
    if not bla:
        table = []
    elif table is None:
        table = XB.bla_table_x(mant, exp2, XB.dcmax_x(W, H, zm, ze))
    sp = spacing_x(zm, ze, H)
    nrows = H if rows is None else len(rows)
    out, total = [], [0, 0, 0]
    for q in range(aa * aa):
        r = perturb_x_de(mant, exp2, X.sample_dc_x(W, H, zm, ze, aa, q, rows), view["max_iter"], table, sp, bailout)
        out.append(tuple(a.reshape(nrows, W) for a in r[:5]))
        total = [a + b for a, b in zip(total, r[5])]
    return out, total


def exact_de_x(view: dict, x: int, y: int, W: int, H: int, max_iter: int = 0, bailout: float = 4.0):
    """(iter, de) of one pixel's sample (0,0) by the direct iteration of z <- z^2 + c, d <- 2 z d + 1 (d_0 = 0) in fixed point
    at F + 64 fraction bits; dc as exact_iter_x forms it, s = zm 2^ze / H as a Fraction; de = |z| log|z| / (|d| s) in pixel
    spacings, 0 for interior.  |d| reaches 1 / zoom and more: it stays a Python integer until the last division."""
    zm, ze = X.zoom_pair(view["zoom"])
    max_iter = max_iter or view["max_iter"]
    G = (view.get("frac_bits") or X.frac_bits_x(view["zoom"])) + 64
    mx, my = R.sample_dc(W, H, zm, 1, 0, rows=[y])
    z2 = Fraction(2) ** ze
    cr = round((Fraction(view["cx"]) + Fraction(float(mx[0, x])) * z2) * (1 << G))
    ci = round((Fraction(view["cy"]) + Fraction(float(my[0, x])) * z2) * (1 << G))
    T = Fraction(float(np.float32(bailout)) ** 2) * (1 << (2 * G))
    sp = Fraction(zm) * z2 / H
    one = 1 << G
    zr = zi = dr = di = sr = si = 0                                # sr, si: the squares the escape test formed
    for i in range(max_iter):
        dr, di = ((2 * (zr * dr - zi * di)) >> G) + one, (2 * (zr * di + zi * dr)) >> G
        zr, zi = ((sr - si) >> G) + cr, ((2 * zr * zi) >> G) + ci
        sr, si = zr * zr, zi * zi
        n2 = sr + si
        if n2 > T:
            zl = math.sqrt(float(Fraction(n2, 1 << (2 * G))))
            dl = Fraction(math.isqrt(dr * dr + di * di), one) * sp
            return i, float(Fraction(zl * math.log(zl)) / dl)
    return max_iter, 0.0
