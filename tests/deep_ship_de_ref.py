"""Distance estimates for deep Burning Ship views (fr_render_deep_ship_de, fr_render_deepx_ship_de): the header's arithmetic
restated operation for operation in fp64 numpy, and the ground truth in Python integers and Fractions.

- ship_l / mandel_l: the linear part L of a plain step at the point (x, y) -- the ship's, and Mandelbrot's for the conformal check;
- perturb_de: deep_ship_bla_ref.perturb_bla (an empty table: deep_ship_ref.perturb's plain path) with the scaled Jacobian
  J = dz/dc * s carried next to the delta; returns (iter, r2, J, z, counts);
- perturb_x_de: deepx_ship_bla_ref.perturb_ship_x_bla (an empty table: deepx_ship_ref.perturb_ship_x) with J as four mantissas
  and one exponent; returns (iter, r2, J, Je, z, counts);
- de_of / de_x_of / deriv_of / deriv_x_of: the two planes from what the loops hand back;
- restate_de / restate_x_de: every sub-sample of a frame (or of its rows), s from the whole frame;
- exact_de: z and dz/dc of one sample iterated directly in Python integers at F + 64 fraction bits, the signs taken from the
  exact values;
- exact_orbit_fraction: the exact orbit of a c in Fractions, for the finite-difference check of the convention.

deep_ship_ref, deep_ship_bla_ref, deepx_ship_ref and deepx_ship_bla_ref supply orbits, sample offsets, folds and tables; none of
them is modified.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import deep_bla_ref as BR
import deep_de_ref as DE
import deep_ref as R
import deep_ship_bla_ref as SB
import deep_ship_ref as S
import deepx_ref as X
import deepx_ship_bla_ref as XSB
import deepx_ship_ref as XS
from deepx_ref import X_THR, X_ZERO, _ld, _norm

def views() -> dict:
    """the views of the tests: SHIP_A and SHIP_B of the fp64 range (zoom a double), the extended ones by name"""
    v = {"A": S.SHIP_A, "B": S.SHIP_B}
    v.update({k: x for k, x in XS.views().items() if k in ("S310", "S400", "TIP400", "TIPY300", "NUC546")})
    return v


def ship_l(wx, wy, x, y):
    """L = [[wx, -wy], [|wy| sgn x, |wx| sgn y]], sgn v = v >= 0 ? 1 : -1; (x, y) carries the signs only"""
    return wx, -wy, np.where(x >= 0.0, np.abs(wy), -np.abs(wy)), np.where(y >= 0.0, np.abs(wx), -np.abs(wx))


def mandel_l(wx, wy, x, y):
    """Mandelbrot's L = [[wx, -wy], [wy, wx]]: with it J is conformal and equals deep_de_ref's D"""
    return wx, -wy, wy, wx


def _lj(L, J):
    """L J without the spacing: the four sums of two products"""
    l11, l12, l21, l22 = L
    j11, j12, j21, j22 = J
    return [l11 * j11 + l12 * j21, l11 * j12 + l12 * j22, l21 * j11 + l22 * j21, l21 * j12 + l22 * j22]


def perturb_de(orbit: np.ndarray, dcx: np.ndarray, dcy: np.ndarray, max_iter: int, table, s, bailout: float = 4.0,
               lin=ship_l, fold: bool = True):
    """The ship's per-sample step with BLA and J.  Plain step: J' = L J + s I at (x, y) = Z_m + dz, s added behind each diagonal
    sum; BLA step: Jij' = (ai1 J1j + ai2 J2j) + bij s; a rebase leaves J alone.  table == []: the plain path.  lin = mandel_l and
    fold = False: Mandelbrot's step and derivative in the same 2x2 form (the conformal check; no table).
    Returns (iter, r2, J, z, counts): J (..., 4) and z (..., 2) of the escaping update for an escaped sample."""
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
    Jout = np.zeros((n, 4), np.float64)
    zout = np.zeros((n, 2), np.float64)
    idx = np.arange(n)
    dzx = np.zeros(n); dzy = np.zeros(n)
    J = [np.zeros(n) for _ in range(4)]
    m = np.zeros(n, np.int64)
    u = np.zeros(n, np.int64)
    counts = [0, 0, 0]
    with np.errstate(all="ignore"):
        while idx.size:
            Zx, Zy = ox[m], oy[m]
            dz2 = dzx * dzx + dzy * dzy
            k = np.zeros(idx.size, np.int64)
            if K:
                r0 = np.float64(BR.EPS) * np.sqrt(Zx * Zx + Zy * Zy)
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
            # the derivative's plain step, from the point before the update
            x = Zx + dzx
            y = Zy + dzy
            P = _lj(lin(x + x, y + y, x, y), J)
            nJ = [P[0] + s, P[1], P[2], P[3] + s]
            if fold:
                fx, fy = S.fold(Zx, dzx), S.fold(Zy, dzy)
                tx = (np.abs(Zx) + np.abs(Zx)) + fx
                ty = (np.abs(Zy) + np.abs(Zy)) + fy
            else:
                fx, fy = dzx, dzy
                tx = (Zx + Zx) + dzx
                ty = (Zy + Zy) + dzy
            nx = (tx * fx - ty * fy) + cx
            ny = (tx * fy + ty * fx) + cy
            if bl.any():
                b = np.nonzero(bl)[0]
                kb = k[b]
                j = (m[b] - 1) >> kb
                E = {q: np.empty(b.size) for q in SB.ELEMS}
                for lvl in np.unique(kb):
                    q_ = kb == lvl
                    T = table[lvl - 1]
                    for q in SB.ELEMS:
                        E[q][q_] = T[q][j[q_]]
                ex, ey, gx, gy = dzx[b], dzy[b], cx[b], cy[b]
                nx[b] = (E["a11"] * ex + E["a12"] * ey) + (E["b11"] * gx + E["b12"] * gy)
                ny[b] = (E["a21"] * ex + E["a22"] * ey) + (E["b21"] * gx + E["b22"] * gy)
                j11, j12, j21, j22 = (v[b] for v in J)
                nJ[0][b] = (E["a11"] * j11 + E["a12"] * j21) + E["b11"] * s
                nJ[1][b] = (E["a11"] * j12 + E["a12"] * j22) + E["b12"] * s
                nJ[2][b] = (E["a21"] * j11 + E["a22"] * j21) + E["b21"] * s
                nJ[3][b] = (E["a21"] * j12 + E["a22"] * j22) + E["b22"] * s
            J = nJ
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
            e = idx[esc]
            it[e] = (u[esc] - 1).astype(np.int32)
            r2out[e] = r2[esc]
            for c in range(4):
                Jout[e, c] = J[c][esc]
            zout[e, 0] = zx[esc]; zout[e, 1] = zy[esc]
            keep = ~esc & (u < max_iter)
            if not keep.all():
                idx, dzx, dzy, m, u, cx, cy = (a[keep] for a in (idx, dzx, dzy, m, u, cx, cy))
                J = [v[keep] for v in J]
    return it.reshape(shape), r2out.reshape(shape), Jout.reshape(shape + (4,)), zout.reshape(shape + (2,)), counts


def gradient(J: np.ndarray, z: np.ndarray, r2: np.ndarray):
    """g = J^T z / |z|: zl = sqrt(r2), ux = zx / zl, uy = zy / zl, g = (J11 ux + J21 uy, J12 ux + J22 uy)"""
    with np.errstate(all="ignore"):
        zl = np.sqrt(r2)
        ux, uy = z[..., 0] / zl, z[..., 1] / zl
        return J[..., 0] * ux + J[..., 2] * uy, J[..., 1] * ux + J[..., 3] * uy


def de_of(it: np.ndarray, r2: np.ndarray, J: np.ndarray, z: np.ndarray, max_iter: int) -> np.ndarray:
    """de = (zl log zl) / sqrt(g.x g.x + g.y g.y), NaN -> 0, interior 0: deep_de_ref.de_of on the gradient"""
    gx, gy = gradient(J, z, r2)
    return DE.de_of(it, r2, gx, gy, max_iter)


def deriv_of(it: np.ndarray, J: np.ndarray, max_iter: int) -> np.ndarray:
    """the deriv plane: (J11, J12, J21, J22) for an escaped sample, zeros for interior"""
    return np.where((it < max_iter)[..., None], J, 0.0)


def restate_de(view: dict, W: int, H: int, aa: int = 1, bailout: float = 4.0, rows=None, orbit=None, bla: bool = False):
    """Every sub-sample of the frame (or of its rows): a list over q of (iter, r2, J, z), and the three counts summed.  s and
    dcmax are those of the whole W x H frame, whatever the rows."""
    if orbit is None:
        orbit = S.reference_orbit(view["cx"], view["cy"], view["zoom"], view["max_iter"], bailout)
    table = SB.bla_table(orbit, SB.dcmax(W, H, view["zoom"])) if bla else []
    sp = DE.spacing(view["zoom"], H)
    out, total = [], [0, 0, 0]
    for q in range(aa * aa):
        dcx, dcy = S.sample_dc(W, H, view["zoom"], aa, q, rows)
        it, r2, J, z, c = perturb_de(orbit, dcx, dcy, view["max_iter"], table, sp, bailout)
        out.append((it, r2, J, z))
        total = [a + b for a, b in zip(total, c)]
    return out, total


# ---- the extended range ---------------------------------------------------------------------------------------------------
def spacing_x(zm: float, ze: int, H: int):
    """s = norm1(zm / H, ze): (sm, es), sm in [0.5, 1)"""
    sm, k = math.frexp(float(np.float64(zm) / np.float64(H)))
    return np.float64(sm), ze + k


def _jset(P, ep, Q, eq):
    """norm4((P, ep) (+) (Q, eq)): Q a list of four mantissas, or a scalar sm for sm I (nothing added off the diagonal)"""
    e = np.maximum(ep, eq)
    if isinstance(Q, list):
        M = [_ld(p, ep - e) + _ld(q, eq - e) for p, q in zip(P, Q)]
    else:
        q = _ld(np.full(P[0].shape, Q), eq - e)
        M = [_ld(P[0], ep - e) + q, _ld(P[1], ep - e), _ld(P[2], ep - e), _ld(P[3], ep - e) + q]
    return XSB._norm4(M, e)


def perturb_x_de(mant, exp2, dc, max_iter: int, table, sm, es: int, bailout: float = 4.0, signs_from_b: bool = False):
    """The ship's two-mode step with BLA on flat sample arrays, and J = (four mantissas, Je) normalised after every update.
    signs_from_b: a WRONG extended step, for the tests only, that takes L's signs from b's mantissas, where a coordinate far
    below the other has lost its sign.
    Returns (iter, r2, J (n, 4), Je (n,), z (n, 2) plain doubles, counts)."""
    omx, omy = np.ascontiguousarray(mant[:, 0]), np.ascontiguousarray(mant[:, 1])
    oe = exp2.astype(np.int64)
    plain = X.decode(mant, exp2)
    opx, opy = np.ascontiguousarray(plain[:, 0]), np.ascontiguousarray(plain[:, 1])
    N = len(oe) - 1
    K = len(table)
    B2 = np.float64(np.float32(bailout)) * np.float64(np.float32(bailout))
    sm = np.float64(sm)
    cx, cy, ec, cpx, cpy = dc
    n = cx.size
    it = np.full(n, max_iter, np.int32)
    r2out = np.zeros(n, np.float64)
    Jout = np.zeros((n, 4), np.float64)
    Jeout = np.full(n, X_ZERO, np.int64)
    zout = np.zeros((n, 2), np.float64)
    idx = np.arange(n)
    dx = np.zeros(n); dy = np.zeros(n)
    ed = np.full(n, X_ZERO, np.int64)
    ext = np.ones(n, bool)
    m = np.zeros(n, np.int64)
    u = np.zeros(n, np.int64)
    J = [np.zeros(n) for _ in range(4)]
    Je = np.full(n, X_ZERO, np.int64)
    counts = [0, 0, 0]

    def put_j(Sel, M, e):
        for c in range(4):
            J[c][Sel] = M[c]
        Je[Sel] = e

    def finish(Sel, mm, nx, ny, en, esc, r2e, ze):
        Wx, Wy, eW = omx[mm], omy[mm], oe[mm]
        ez = np.maximum(eW, en)
        zx = _ld(Wx, eW - ez) + _ld(nx, en - ez)
        zy = _ld(Wy, eW - ez) + _ld(ny, en - ez)
        r2 = zx * zx + zy * zy
        r2d = _ld(r2, 2 * ez)
        es_ = r2d > B2
        n2 = nx * nx + ny * ny
        reb = ~es_ & ((r2 < _ld(n2, 2 * (en - ez))) | (mm == N))
        ax, ay, ea = _norm(np.where(reb, zx, nx), np.where(reb, zy, ny), np.where(reb, ez, en))
        stay = ea <= X_THR
        dx[Sel] = np.where(stay, ax, _ld(ax, np.where(stay, 0, ea)))
        dy[Sel] = np.where(stay, ay, _ld(ay, np.where(stay, 0, ea)))
        ed[Sel] = ea
        ext[Sel] = stay
        m[Sel] = np.where(reb, 0, mm)
        esc[Sel] = es_
        r2e[Sel] = r2d
        ze[Sel, 0] = _ld(zx, np.where(es_, ez, 0)); ze[Sel, 1] = _ld(zy, np.where(es_, ez, 0))

    with np.errstate(all="ignore"):
        while idx.size:
            esc = np.zeros(idx.size, bool)
            r2e = np.zeros(idx.size)
            ze = np.zeros((idx.size, 2))
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
                for lvl in range(K, 0, -1):
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
                    el = {q: np.empty(b.size) for q in SB.ELEMS}
                    ea = np.empty(b.size, np.int64); eb = np.empty(b.size, np.int64)
                    for lvl in np.unique(kb):
                        q_ = kb == lvl
                        T = table[lvl - 1]
                        for q in SB.ELEMS:
                            el[q][q_] = T[q][j[q_]]
                        ea[q_], eb[q_] = T["ea"][j[q_]], T["eb"][j[q_]]
                    # J' = norm4((A J, A.e + J.e) (+) (B sm, B.e + es))
                    A = (el["a11"], el["a12"], el["a21"], el["a22"])
                    M, e = _jset(_lj(A, [v[Bl] for v in J]), ea + Je[Bl],
                                 [el["b11"] * sm, el["b12"] * sm, el["b21"] * sm, el["b22"] * sm], eb + es)
                    x, y, e_ = qx[b], qy[b], qe[b]
                    gx, gy, ge = cx[Bl], cy[Bl], ec[Bl]
                    px, py, ep = el["a11"] * x + el["a12"] * y, el["a21"] * x + el["a22"] * y, ea + e_
                    sx, sy, eq = el["b11"] * gx + el["b12"] * gy, el["b21"] * gx + el["b22"] * gy, eb + ge
                    en = np.maximum(ep, eq)
                    nx = _ld(px, ep - en) + _ld(sx, eq - en)
                    ny = _ld(py, ep - en) + _ld(sy, eq - en)
                    put_j(Bl, M, e)
                    finish(Bl, mc[b] + np.left_shift(1, kb), nx, ny, en, esc, r2e, ze)
            bl = k > 0
            E = np.nonzero(ext & ~bl)[0]
            P = np.nonzero(~ext & ~bl)[0]
            if E.size:
                mm = m[E]
                Zx, Zy, eZ = omx[mm], omy[mm], oe[mm]
                x, y, e = dx[E], dy[E], ed[E]
                # b = (Z_m, eZ) (+) (dz, ed) at eb; L's magnitudes from b's mantissas, its signs from fold_x's w, the sum in the
                # delta's frame; J' = norm4((L J, eb + 1 + J.e) (+) (sm I, es))
                eb = np.maximum(eZ, e)
                bx = _ld(Zx, eZ - eb) + _ld(x, e - eb)
                by = _ld(Zy, eZ - eb) + _ld(y, e - eb)
                sgx, sgy = (bx, by) if signs_from_b else (_ld(Zx, eZ - e) + x, _ld(Zy, eZ - e) + y)
                M, eJ = _jset(_lj(ship_l(bx, by, sgx, sgy), [v[E] for v in J]), eb + 1 + Je[E], sm, es)
                fx, _ = XS.fold_x(Zx, eZ, x, e)
                fy, _ = XS.fold_x(Zy, eZ, y, e)
                et = np.maximum(eZ + 1, e)
                tx = _ld(np.abs(Zx), eZ + 1 - et) + _ld(fx, e - et)
                ty = _ld(np.abs(Zy), eZ + 1 - et) + _ld(fy, e - et)
                px = tx * fx - ty * fy
                py = tx * fy + ty * fx
                ep = et + e
                en = np.maximum(ep, ec[E])
                nx = _ld(px, ep - en) + _ld(cx[E], ec[E] - en)
                ny = _ld(py, ep - en) + _ld(cy[E], ec[E] - en)
                put_j(E, M, eJ)
                finish(E, mm + 1, nx, ny, en, esc, r2e, ze)
            if P.size:
                mm = m[P]
                Zx, Zy = opx[mm], opy[mm]
                x, y = dx[P], dy[P]
                # L from the plain doubles, the product at J.e
                px_ = Zx + x
                py_ = Zy + y
                M, eJ = _jset(_lj(ship_l(px_ + px_, py_ + py_, px_, py_), [v[P] for v in J]), Je[P], sm, es)
                fx, fy = S.fold(Zx, x), S.fold(Zy, y)
                tx = (np.abs(Zx) + np.abs(Zx)) + fx
                ty = (np.abs(Zy) + np.abs(Zy)) + fy
                nx = (tx * fx - ty * fy) + cpx[P]
                ny = (tx * fy + ty * fx) + cpy[P]
                mm = mm + 1
                zx = opx[mm] + nx
                zy = opy[mm] + ny
                r2 = zx * zx + zy * zy
                es_ = r2 > B2
                reb = ~es_ & ((r2 < nx * nx + ny * ny) | (mm == N))
                ax = np.where(reb, zx, nx)
                ay = np.where(reb, zy, ny)
                small = np.maximum(np.abs(ax), np.abs(ay)) < X._THR
                bx, by, be = _norm(ax, ay, np.zeros(P.size, np.int64))
                dx[P] = np.where(small, bx, ax)
                dy[P] = np.where(small, by, ay)
                ed[P] = be
                ext[P] = small
                m[P] = np.where(reb, 0, mm)
                esc[P] = es_
                r2e[P] = r2
                ze[P, 0] = zx; ze[P, 1] = zy
                put_j(P, M, eJ)
            step = np.where(bl, np.left_shift(1, k), 1)
            counts[0] += int((~bl).sum())
            counts[1] += int(bl.sum())
            counts[2] += int(step[bl].sum())
            u = u + step
            e = idx[esc]
            it[e] = (u[esc] - 1).astype(np.int32)
            r2out[e] = r2e[esc]
            for c in range(4):
                Jout[e, c] = J[c][esc]
            Jeout[e] = Je[esc]
            zout[e] = ze[esc]
            keep = ~esc & (u < max_iter)
            if not keep.all():
                idx, dx, dy, ed, ext, m, u, Je = (a[keep] for a in (idx, dx, dy, ed, ext, m, u, Je))
                J = [v[keep] for v in J]
                cx, cy, ec, cpx, cpy = cx[keep], cy[keep], ec[keep], cpx[keep], cpy[keep]
    return it, r2out, Jout, Jeout, zout, counts


def de_x_of(it, r2, J, Je, z, max_iter: int) -> np.ndarray:
    """de = ldexp(de_of(r2, g of the mantissas), -J.e): finite at any depth"""
    d = de_of(it, r2, J, z, max_iter)
    return _ld(d, np.where(it < max_iter, -Je, 0))


def deriv_x_of(it, J, Je, max_iter: int) -> np.ndarray:
    """ldexp(Jij, J.e), saturating outside a double's range; zeros for interior"""
    e = it < max_iter
    with np.errstate(all="ignore"):
        return np.where(e[..., None], _ld(J, np.where(e, Je, 0)[..., None]), 0.0)


def restate_x_de(view: dict, W: int, H: int, aa: int = 1, bailout: float = 4.0, rows=None, orbit=None, bla: bool = False,
                 pixels=None, signs_from_b: bool = False):
    """Every sub-sample of the rows: a list over q of (iter, r2, J, Je, z) planes, and the three counts summed.
    pixels = (ys, xs): those samples only, flat."""
    mant, exp2 = orbit if orbit is not None else XS.orbit_of(view, bailout)
    zm, ze = X.zoom_pair(view["zoom"])
    table = XSB.bla_table_ship_x(mant, exp2, XSB.dcmax_ship_x(W, H, zm, ze)) if bla else []
    sm, es = spacing_x(zm, ze, H)
    nrows = H if rows is None else len(rows)
    out, total = [], [0, 0, 0]
    for q in range(aa * aa):
        dc = XS.sample_dc_ship_x(W, H, zm, ze, aa, q, rows)
        if pixels is not None:
            sel = np.asarray(pixels[0]) * W + np.asarray(pixels[1])
            dc = tuple(a[sel] for a in dc)
        it, r2, J, Je, z, c = perturb_x_de(mant, exp2, dc, view["max_iter"], table, sm, es, bailout, signs_from_b)
        if pixels is None:
            it, r2, Je = it.reshape(nrows, W), r2.reshape(nrows, W), Je.reshape(nrows, W)
            J, z = J.reshape(nrows, W, 4), z.reshape(nrows, W, 2)
        out.append((it, r2, J, Je, z))
        total = [a + b for a, b in zip(total, c)]
    return out, total


# ---- ground truth -----------------------------------------------------------------------------------------------------------
def exact_de(view: dict, x: int, y: int, W: int, H: int, bailout: float = 4.0):
    """(iter, de) of one pixel's sample (0,0): z <- (|x| + i|y|)^2 + c and d <- L d + I (d_0 = 0, d = dz/dc as a 2x2 integer
    matrix) iterated directly in fixed point at F + 64 fraction bits, the signs of L from the exact z.  c = centre + dc with dc
    the double(s) the kernel forms, exactly.  de = |z| log|z| / (|d^T z / |z|| s) in pixel spacings, 0 for interior.  The view's
    zoom is a double (fp64 range) or a decimal string (extended)."""
    if isinstance(view["zoom"], str):
        zm, ze = X.zoom_pair(view["zoom"])
        G = XS.frac_bits_of(view) + 64
        mx, my = S.sample_dc(W, H, zm, 1, 0, rows=[y])
        sc = Fraction(2) ** ze
        s = Fraction(float(np.float64(zm) / np.float64(H))) * sc
    else:
        G = R.frac_bits(view["zoom"]) + 64
        mx, my = S.sample_dc(W, H, view["zoom"], 1, 0, rows=[y])
        sc = Fraction(1)
        s = Fraction(float(DE.spacing(view["zoom"], H)))
    cr = round((Fraction(view["cx"]) + Fraction(float(mx[0, x])) * sc) * (1 << G))
    ci = round((Fraction(view["cy"]) + Fraction(float(my[0, x])) * sc) * (1 << G))
    T = Fraction(float(np.float32(bailout)) ** 2) * (1 << (2 * G))
    one = 1 << G
    zr = zi = 0
    d11 = d12 = d21 = d22 = 0
    for i in range(view["max_iter"]):
        sx, sy = (1 if zr >= 0 else -1), (1 if zi >= 0 else -1)
        l11, l12, l21, l22 = 2 * zr, -2 * zi, 2 * abs(zi) * sx, 2 * abs(zr) * sy
        d11, d12, d21, d22 = (((l11 * d11 + l12 * d21) >> G) + one, (l11 * d12 + l12 * d22) >> G,
                              (l21 * d11 + l22 * d21) >> G, ((l21 * d12 + l22 * d22) >> G) + one)
        zr, zi = ((zr * zr - zi * zi) >> G) + cr, ((2 * abs(zr) * abs(zi)) >> G) + ci
        n2 = zr * zr + zi * zi
        if n2 > T:
            zl = math.sqrt(float(Fraction(n2, 1 << (2 * G))))
            gx, gy = d11 * zr + d21 * zi, d12 * zr + d22 * zi          # d^T z, scale 2^(2G); / |z| below
            gl = Fraction(math.isqrt(gx * gx + gy * gy), math.isqrt(n2) << G) * s
            return i, float(Fraction(zl * math.log(zl)) / gl)
    return view["max_iter"], 0.0


def exact_orbit_fraction(cx: Fraction, cy: Fraction, n: int):
    """z_n of the ship's map from 0, exactly"""
    x = y = Fraction(0)
    for _ in range(n):
        x, y = x * x - y * y + cx, 2 * abs(x) * abs(y) + cy
    return x, y


def jacobian_fraction(cx: Fraction, cy: Fraction, n: int):
    """dz_n/dc by the recurrence of the header (J / s), exactly: d' = L d + I, L from the exact z before the update"""
    x = y = Fraction(0)
    d = [Fraction(0)] * 4
    for _ in range(n):
        sx, sy = (1 if x >= 0 else -1), (1 if y >= 0 else -1)
        L = (2 * x, -2 * y, 2 * abs(y) * sx, 2 * abs(x) * sy)
        d = [L[0] * d[0] + L[1] * d[2] + 1, L[0] * d[1] + L[1] * d[3], L[2] * d[0] + L[3] * d[2], L[2] * d[1] + L[3] * d[3] + 1]
        x, y = x * x - y * y + cx, 2 * abs(x) * abs(y) + cy
    return d
