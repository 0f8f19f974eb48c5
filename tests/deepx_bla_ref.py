"""Extended views with bilinear approximation (fr_render_deepx with FR_FLAG_DEEPX_BLA): the table build and the stepping
of the header, restated operation for operation in numpy, vectorised over samples.

- dcmax_x / bla_table_x: the constants and the levels k = 1 .. K of the extended table, as the device builds them;
- perturb_x_bla: the two-mode step of deepx_ref.perturb_x with BLA steps in both modes; returns the (iter, r2) planes and the
  three step counts;
- restate_x_bla: every sub-sample of a frame (or of its rows), the counts summed (fr_ctx_last_deepx_steps).

deepx_ref.py supplies the orbit, the sample offsets and the helpers of the extended arithmetic (_norm, _ld); the level
logic is deep_bla_ref's.
"""
from __future__ import annotations

import numpy as np

import deep_bla_ref as BR
import deepx_ref as X
from deepx_ref import X_THR, X_ZERO, _ld, _norm

E_LIM = 1 << 27              # an entry whose A or B exponent leaves [-E_LIM, E_LIM] is void
R_BITS = 24                  # a stored radius keeps the top 24 bits of its mantissa (toward zero): a float


def _norm1(v, e):
    """an extended real normalised: v into [0.5, 1); zero gets X_ZERO"""
    m, k = np.frexp(v)
    return m, np.where(v == 0.0, X_ZERO, e + k.astype(np.int64))


def _abs_x(x, y, e):
    """|w| of a normalised extended complex: (sqrt(x*x + y*y), e), normalised"""
    return _norm1(np.sqrt(x * x + y * y), e)


def _trunc(v):
    """the top R_BITS bits of a mantissa in [0.5, 1) or 0: what a float holds, rounded toward zero"""
    mask = np.uint64(~((1 << (53 - R_BITS)) - 1) & 0xFFFFFFFFFFFFFFFF)
    return (np.ascontiguousarray(v, np.float64).view(np.uint64) & mask).view(np.float64)


def dcmax_x(W: int, H: int, zm: float, ze: int):
    """(1.0000001 * (0.5 * zm)) * sqrt((W/H)*(W/H) + 1) of the whole frame with the exponent ze, normalised: (v, e)"""
    a = np.float64(W) / np.float64(H)
    v = (np.float64(1.0000001) * (np.float64(0.5) * np.float64(zm))) * np.sqrt(a * a + np.float64(1.0))
    m, e = _norm1(np.array([v]), np.array([ze], np.int64))
    return float(m[0]), int(e[0])


def bla_table_x(mant: np.ndarray, exp2: np.ndarray, dcm):
    """Levels 1 .. K: a list of dicts (index k - 1) with arrays rv, re (the radius), ax, ay, ea, bx, by, eb over the
    entries j of the level, entry j covering the 2^k steps from m = 1 + j * 2^k"""
    N = len(exp2) - 1
    K = BR.levels(N)
    if K == 0:
        return []
    dv, de = np.float64(dcm[0]), np.int64(dcm[1])
    with np.errstate(all="ignore"):
        zx, zy = mant[1:N, 0].copy(), mant[1:N, 1].copy()           # the single steps m = 1 .. N - 1
        ze = exp2[1:N].astype(np.int64)
        ax, ay, ea = _norm(zx, zy, ze + 1)
        bx, by, eb = _norm(np.ones_like(zx), np.zeros_like(zx), np.zeros_like(ze))
        nx, ny, ne = _norm(zx, zy, ze)
        rv, re = _abs_x(nx, ny, ne)
        re = np.where(rv == 0.0, X_ZERO, re - 53)
        prev = dict(rv=rv, re=re, ax=ax, ay=ay, ea=ea, bx=bx, by=by, eb=eb)
        out = []
        for k in range(1, K + 1):
            cnt = (N - 1) >> k
            x = {key: v[0:2 * cnt:2] for key, v in prev.items()}
            y = {key: v[1:2 * cnt:2] for key, v in prev.items()}
            ax, ay, ea = _norm(y["ax"] * x["ax"] - y["ay"] * x["ay"], y["ax"] * x["ay"] + y["ay"] * x["ax"], y["ea"] + x["ea"])
            px = y["ax"] * x["bx"] - y["ay"] * x["by"]
            py = y["ax"] * x["by"] + y["ay"] * x["bx"]
            e1 = y["ea"] + x["eb"]
            e = np.maximum(e1, y["eb"])
            bx, by, eb = _norm(_ld(px, e1 - e) + _ld(y["bx"], y["eb"] - e), _ld(py, e1 - e) + _ld(y["by"], y["eb"] - e), e)
            bv, be = _abs_x(x["bx"], x["by"], x["eb"])
            pv, pe = bv * dv, be + de
            av, ae = _abs_x(x["ax"], x["ay"], x["ea"])
            e = np.maximum(y["re"], pe)
            t = (_ld(y["rv"], y["re"] - e) - _ld(pv, pe - e)) / av
            ok = (t > 0.0) & np.isfinite(t)
            rv, re = _norm1(np.where(ok, t, 0.0), e - ae)
            less = (re < x["re"]) | ((re == x["re"]) & (rv < x["rv"]))
            rv, re = np.where(less, rv, x["rv"]), np.where(less, re, x["re"])
            void = (np.abs(ea) > E_LIM) | (np.abs(eb) > E_LIM)
            rv, re = np.where(void, 0.0, rv), np.where(void, X_ZERO, re)
            ax, ay, ea = np.where(void, 0.0, ax), np.where(void, 0.0, ay), np.where(void, X_ZERO, ea)
            bx, by, eb = np.where(void, 0.0, bx), np.where(void, 0.0, by), np.where(void, X_ZERO, eb)
            prev = dict(rv=_trunc(rv), re=re, ax=ax, ay=ay, ea=ea, bx=bx, by=by, eb=eb)
            out.append(prev)
    return out


def perturb_x_bla(mant, exp2, dc, max_iter: int, table, bailout: float = 4.0):
    """The two-mode step of the header with BLA on flat sample arrays.  Returns (iter, r2, counts): counts = [plain +
    extended single steps, BLA steps, updates skipped] over the samples."""
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

    def finish(S, mm, nx, ny, en, esc, r2e):
        """z = Z_m (+) n, the escape test, the rebase rule, norm and the mode rule of the EXTENDED step, for the samples S"""
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
        dx[S] = np.where(stay, ax, _ld(ax, np.where(stay, 0, ea)))
        dy[S] = np.where(stay, ay, _ld(ay, np.where(stay, 0, ea)))
        ed[S] = ea
        ext[S] = stay
        m[S] = np.where(reb, 0, mm)
        esc[S] = es
        r2e[S] = r2d

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
                    ax = np.empty(b.size); ay = np.empty(b.size); bx = np.empty(b.size); by = np.empty(b.size)
                    ea = np.empty(b.size, np.int64); eb = np.empty(b.size, np.int64)
                    for lvl in np.unique(kb):
                        s = kb == lvl
                        T = table[lvl - 1]
                        ax[s], ay[s], ea[s] = T["ax"][j[s]], T["ay"][j[s]], T["ea"][j[s]]
                        bx[s], by[s], eb[s] = T["bx"][j[s]], T["by"][j[s]], T["eb"][j[s]]
                    x, y, e = qx[b], qy[b], qe[b]
                    gx, gy, ge = cx[Bl], cy[Bl], ec[Bl]
                    px, py, ep = ax * x - ay * y, ax * y + ay * x, ea + e
                    sx, sy, es_ = bx * gx - by * gy, bx * gy + by * gx, eb + ge
                    en = np.maximum(ep, es_)
                    nx = _ld(px, ep - en) + _ld(sx, es_ - en)
                    ny = _ld(py, ep - en) + _ld(sy, es_ - en)
                    finish(Bl, mc[b] + np.left_shift(1, kb), nx, ny, en, esc, r2e)
            bl = k > 0
            E = np.nonzero(ext & ~bl)[0]
            P = np.nonzero(~ext & ~bl)[0]
            # a BLA step may have changed ext of its own lanes: E and P are taken from the single-step lanes only,
            # whose mode no BLA step touched (bl lanes are excluded by index)
            if E.size:
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
                finish(E, mm + 1, nx, ny, en, esc, r2e)
            if P.size:
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
    return bla_table_x(orbit[0], orbit[1], dcmax_x(W, H, zm, ze))


def restate_x_bla(view: dict, W: int, H: int, aa: int = 1, bailout: float = 4.0, rows=None, orbit=None, table=None):
    """Every sub-sample of the frame (or of its rows): a list over s of (iter, r2) planes, and the three counts summed.
    dcmax is that of the whole W x H frame, whatever the rows."""
    mant, exp2 = orbit if orbit is not None else X.orbit_of(view, bailout)
    zm, ze = X.zoom_pair(view["zoom"])
    if table is None:
        table = bla_table_x(mant, exp2, dcmax_x(W, H, zm, ze))
    nrows = H if rows is None else len(rows)
    out, total = [], [0, 0, 0]
    for s in range(aa * aa):
        it, r2, c = perturb_x_bla(mant, exp2, X.sample_dc_x(W, H, zm, ze, aa, s, rows), view["max_iter"], table, bailout)
        out.append((it.reshape(nrows, W), r2.reshape(nrows, W)))
        total = [a + b for a, b in zip(total, c)]
    return out, total
