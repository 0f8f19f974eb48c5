"""Extended Burning Ship views with bilinear approximation (fr_render_deepx_ship with FR_FLAG_DEEPX_SHIP_BLA): the table
build and the stepping of the header, restated operation for operation in numpy, vectorised over samples.

- dcmax_ship_x / bla_table_ship_x: the constants and the levels k = 1 .. K of the extended ship table, as the device builds
  them;
- perturb_ship_x_bla: the two-mode step of deepx_ship_ref.perturb_ship_x with BLA steps in both modes; returns the (iter, r2)
  planes and the three step counts;
- restate_ship_x_bla: every sub-sample of a frame (or of its rows), the counts summed (fr_ctx_last_deepx_ship_steps).

deepx_ship_ref.py supplies the orbit, the sample offsets and the two-mode single step; deepx_bla_ref.py the helpers of the
extended table (_norm1, _trunc, the void limit); deep_ship_bla_ref.py the element order; the level logic is deep_bla_ref's.
"""
from __future__ import annotations

import numpy as np

import deep_bla_ref as BR
import deep_ship_ref as S
import deepx_ref as X
import deepx_ship_ref as XS
from deep_ship_bla_ref import ELEMS
from deepx_bla_ref import E_LIM, _norm1, _trunc
from deepx_ref import X_THR, X_ZERO, _ld, _norm

A_ELEMS, B_ELEMS = ELEMS[:4], ELEMS[4:]


def _norm4(m, e):
    """norm4 of the header: four mantissas (a list of arrays) normalised on the largest of them; the zero matrix gets X_ZERO"""
    mx = np.maximum(np.maximum(np.abs(m[0]), np.abs(m[1])), np.maximum(np.abs(m[2]), np.abs(m[3])))
    _, k = np.frexp(mx)
    k = k.astype(np.int64)
    return [_ld(v, -k) for v in m], np.where(mx == 0.0, X_ZERO, e + k)


def _less(v, e, w, f):
    """(v, e) < (w, f) on normalised extended reals; the zero's exponent X_ZERO is below every other"""
    return (e < f) | ((e == f) & (v < w))


def dcmax_ship_x(W: int, H: int, zm: float, ze: int):
    """deep_ship_bla_ref.dcmax's formula on the zoom's mantissa with the exponent ze, normalised: (v, e)"""
    f = np.float64
    a = f(W) / f(H)
    hx = f(0.5) + f(0.5) / (f(W) * f(W))
    hy = f(0.5) + f(0.5) / (f(W) * f(H))
    ex = hx * a
    v = (f(1.0000001) * f(zm)) * np.sqrt(ex * ex + hy * hy)
    m, e = _norm1(np.array([v]), np.array([ze], np.int64))
    return float(m[0]), int(e[0])


def single_steps_x(mant: np.ndarray, exp2: np.ndarray) -> dict:
    """The single steps m = 1 .. N - 1 (never stored on the device): A = norm4(X, -Y, |Y| sgn X, |X| sgn Y, eZ + 1),
    B = norm4(1, 0, 0, 1, 0), r = 2^-53 |norm(Z_m)| capped by |X| and |Y| as extended reals"""
    N = len(exp2) - 1
    Xm, Ym = mant[1:N, 0].copy(), mant[1:N, 1].copy()
    eZ = exp2[1:N].astype(np.int64)
    sx = np.where(Xm >= 0.0, 1.0, -1.0)
    sy = np.where(Ym >= 0.0, 1.0, -1.0)
    aX, aY = np.abs(Xm), np.abs(Ym)
    A, ea = _norm4([Xm, -Ym, aY * sx, aX * sy], eZ + 1)
    one, zero = np.ones_like(Xm), np.zeros_like(Xm)
    B, eb = _norm4([one, zero, zero, one], np.zeros_like(eZ))
    nx, ny, ne = _norm(Xm, Ym, eZ)
    rv, re = _norm1(np.sqrt(nx * nx + ny * ny), ne)
    re = np.where(rv == 0.0, X_ZERO, re - 53)
    for c in (aX, aY):
        cv, ce = _norm1(c, eZ)
        less = _less(rv, re, cv, ce)
        rv, re = np.where(less, rv, cv), np.where(less, re, ce)
    out = dict(rv=rv, re=re, ea=ea, eb=eb)
    out.update(zip(A_ELEMS, A))
    out.update(zip(B_ELEMS, B))
    return out


def bla_table_ship_x(mant: np.ndarray, exp2: np.ndarray, dcm):
    """Levels 1 .. K: a list of dicts (index k - 1) with arrays rv, re (the stored radius), the eight mantissas of ELEMS and
    ea, eb over the entries j of the level, entry j covering the 2^k steps from m = 1 + j * 2^k"""
    N = len(exp2) - 1
    K = BR.levels(N)
    if K == 0:
        return []
    dv, de = np.float64(dcm[0]), np.int64(dcm[1])
    with np.errstate(all="ignore"):
        prev = single_steps_x(mant, exp2)
        out = []
        for k in range(1, K + 1):
            cnt = (N - 1) >> k
            x = {key: v[0:2 * cnt:2] for key, v in prev.items()}
            y = {key: v[1:2 * cnt:2] for key, v in prev.items()}
            A, ea = _norm4([y["a11"] * x["a11"] + y["a12"] * x["a21"], y["a11"] * x["a12"] + y["a12"] * x["a22"],
                            y["a21"] * x["a11"] + y["a22"] * x["a21"], y["a21"] * x["a12"] + y["a22"] * x["a22"]],
                           y["ea"] + x["ea"])
            P = [y["a11"] * x["b11"] + y["a12"] * x["b21"], y["a11"] * x["b12"] + y["a12"] * x["b22"],
                 y["a21"] * x["b11"] + y["a22"] * x["b21"], y["a21"] * x["b12"] + y["a22"] * x["b22"]]
            e1 = y["ea"] + x["eb"]
            e = np.maximum(e1, y["eb"])
            B, eb = _norm4([_ld(p, e1 - e) + _ld(y[q], y["eb"] - e) for p, q in zip(P, B_ELEMS)], e)
            bv, be = _norm1(np.sqrt((x["b11"] * x["b11"] + x["b12"] * x["b12"]) + (x["b21"] * x["b21"] + x["b22"] * x["b22"])),
                            x["eb"])
            av, ae = _norm1(np.sqrt(x["a11"] * x["a11"] + x["a21"] * x["a21"]), x["ea"])
            pv, pe = bv * dv, be + de
            e = np.maximum(y["re"], pe)
            t = (_ld(y["rv"], y["re"] - e) - _ld(pv, pe - e)) / av
            ok = (t > 0.0) & np.isfinite(t)
            rv, re = _norm1(np.where(ok, t, 0.0), e - ae)
            less = _less(rv, re, x["rv"], x["re"])
            rv, re = np.where(less, rv, x["rv"]), np.where(less, re, x["re"])
            void = (np.abs(ea) > E_LIM) | (np.abs(eb) > E_LIM)
            rv, re = np.where(void, 0.0, rv), np.where(void, X_ZERO, re)
            prev = dict(rv=_trunc(rv), re=re, ea=np.where(void, X_ZERO, ea), eb=np.where(void, X_ZERO, eb))
            prev.update((q, np.where(void, 0.0, v)) for q, v in zip(A_ELEMS, A))
            prev.update((q, np.where(void, 0.0, v)) for q, v in zip(B_ELEMS, B))
            out.append(prev)
    return out


def perturb_ship_x_bla(mant, exp2, dc, max_iter: int, table, bailout: float = 4.0):
    """The ship's two-mode step with BLA on flat sample arrays.  Returns (iter, r2, counts): counts = [plain + extended single
    steps, BLA steps, updates skipped] over the samples."""
    omx, omy = np.ascontiguousarray(mant[:, 0]), np.ascontiguousarray(mant[:, 1])
    oe = exp2.astype(np.int64)
    plain = X.decode(mant, exp2)
    opx, opy = np.ascontiguousarray(plain[:, 0]), np.ascontiguousarray(plain[:, 1])
    N = len(oe) - 1
    K = len(table)
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
    u = np.zeros(n, np.int64)
    counts = [0, 0, 0]

    def finish(Sel, mm, nx, ny, en, esc, r2e):
        """z = Z_m (+) n, the escape test, the rebase rule, norm and the mode rule of the EXTENDED step, for the samples Sel"""
        Wx, Wy, eW = omx[mm], omy[mm], oe[mm]
        ez = np.maximum(eW, en)
        zx = _ld(Wx, eW - ez) + _ld(nx, en - ez)
        zy = _ld(Wy, eW - ez) + _ld(ny, en - ez)
        r2 = zx * zx + zy * zy
        r2d = _ld(r2, 2 * ez)
        es = r2d > B2
        n2 = nx * nx + ny * ny
        reb = ~es & ((r2 < _ld(n2, 2 * (en - ez))) | (mm == N))
        ax, ay, ea = _norm(np.where(reb, zx, nx), np.where(reb, zy, ny), np.where(reb, ez, en))
        stay = ea <= X_THR
        dx[Sel] = np.where(stay, ax, _ld(ax, np.where(stay, 0, ea)))
        dy[Sel] = np.where(stay, ay, _ld(ay, np.where(stay, 0, ea)))
        ed[Sel] = ea
        ext[Sel] = stay
        m[Sel] = np.where(reb, 0, mm)
        esc[Sel] = es
        r2e[Sel] = r2d

    with np.errstate(all="ignore"):
        while idx.size:
            esc = np.zeros(idx.size, bool)
            r2e = np.zeros(idx.size)
            k = np.zeros(idx.size, np.int64)
            cand = np.nonzero(m >= 1)[0] if K else np.zeros(0, np.int64)
            if cand.size:
                # dz as a normalised extended number: an extended lane has it, a plain lane forms norm(dz.x, dz.y, 0)
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
                    el = {q: np.empty(b.size) for q in ELEMS}
                    ea = np.empty(b.size, np.int64); eb = np.empty(b.size, np.int64)
                    for lvl in np.unique(kb):
                        s = kb == lvl
                        T = table[lvl - 1]
                        for q in ELEMS:
                            el[q][s] = T[q][j[s]]
                        ea[s], eb[s] = T["ea"][j[s]], T["eb"][j[s]]
                    x, y, e = qx[b], qy[b], qe[b]
                    gx, gy, ge = cx[Bl], cy[Bl], ec[Bl]
                    px, py, ep = el["a11"] * x + el["a12"] * y, el["a21"] * x + el["a22"] * y, ea + e
                    sx, sy, es_ = el["b11"] * gx + el["b12"] * gy, el["b21"] * gx + el["b22"] * gy, eb + ge
                    en = np.maximum(ep, es_)
                    nx = _ld(px, ep - en) + _ld(sx, es_ - en)
                    ny = _ld(py, ep - en) + _ld(sy, es_ - en)
                    finish(Bl, mc[b] + np.left_shift(1, kb), nx, ny, en, esc, r2e)
            bl = k > 0
            # E and P are the single-step lanes in the mode they had BEFORE this trip: a BLA step may have changed ext of its
            # own lanes, and those are excluded by bl
            E = np.nonzero(ext & ~bl)[0]
            P = np.nonzero(~ext & ~bl)[0]
            if E.size:
                mm = m[E]
                Zx, Zy, eZ = omx[mm], omy[mm], oe[mm]
                x, y, e = dx[E], dy[E], ed[E]
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
                finish(E, mm + 1, nx, ny, en, esc, r2e)
            if P.size:
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
                ax = np.where(reb, zx, nx)
                ay = np.where(reb, zy, ny)
                small = np.maximum(np.abs(ax), np.abs(ay)) < X._THR
                bx, by, be = _norm(ax, ay, np.zeros(P.size, np.int64))
                dx[P] = np.where(small, bx, ax)
                dy[P] = np.where(small, by, ay)
                ed[P] = be
                ext[P] = small
                m[P] = np.where(reb, 0, mm)
                esc[P] = es
                r2e[P] = r2
            step = np.where(bl, np.left_shift(1, k), 1)
            counts[0] += int((~bl).sum())
            counts[1] += int(bl.sum())
            counts[2] += int(step[bl].sum())
            u = u + step
            it[idx[esc]] = (u[esc] - 1).astype(np.int32)
            r2out[idx[esc]] = r2e[esc]
            keep = ~esc & (u < max_iter)
            if not keep.all():
                idx, dx, dy, ed, ext, m, u = idx[keep], dx[keep], dy[keep], ed[keep], ext[keep], m[keep], u[keep]
                cx, cy, ec, cpx, cpy = cx[keep], cy[keep], ec[keep], cpx[keep], cpy[keep]
    return it, r2out, counts


def table_of(view: dict, W: int, H: int, orbit):
    zm, ze = X.zoom_pair(view["zoom"])
    return bla_table_ship_x(orbit[0], orbit[1], dcmax_ship_x(W, H, zm, ze))


def restate_ship_x_bla(view: dict, W: int, H: int, aa: int = 1, bailout: float = 4.0, rows=None, orbit=None, table=None):
    """Every sub-sample of the frame (or of its rows): a list over s of (iter, r2) planes, and the three counts summed.
    dcmax is that of the whole W x H frame, whatever the rows."""
    mant, exp2 = orbit if orbit is not None else XS.orbit_of(view, bailout)
    zm, ze = X.zoom_pair(view["zoom"])
    if table is None:
        table = bla_table_ship_x(mant, exp2, dcmax_ship_x(W, H, zm, ze))
    nrows = H if rows is None else len(rows)
    out, total = [], [0, 0, 0]
    for s in range(aa * aa):
        dc = XS.sample_dc_ship_x(W, H, zm, ze, aa, s, rows)
        it, r2, c = perturb_ship_x_bla(mant, exp2, dc, view["max_iter"], table, bailout)
        out.append((it.reshape(nrows, W), r2.reshape(nrows, W)))
        total = [a + b for a, b in zip(total, c)]
    return out, total
