"""Deep Julia views with bilinear approximation (fr_render_deep_julia with FR_FLAG_DEEP_JULIA_BLA, fr_render_deepx_julia with
FR_FLAG_DEEPX_JULIA_BLA): the two tables and the stepping of the header, restated operation for operation in numpy, next to
deep_bla_ref / deepx_bla_ref and built on deep_julia_ref.

- bla_tables / bla_tables_x: the (Q, P) pair of tables -- levels k = 1 .. K each, B-less -- as the device builds them;
  flat / flat_x: a pair in the order of the device buffers (Q's entries, then P's);
- perturb_bla / perturb_x_bla: the two-orbit per-sample step with BLA on the sample's current orbit and table;
- restate_bla / restate_x_bla: every sub-sample of a frame: the (iter, r2) planes and the three counts
  (fr_ctx_last_deep_julia_steps / fr_ctx_last_deepx_julia_steps); stats receives the BLA steps taken on Q and on P;
- precritical_centre and the view PRECRIT60: a centre whose orbit passes 0, so that samples reach Q with a squared delta.
"""
from __future__ import annotations

import decimal
import functools

import numpy as np

import deep_bla_ref as BR
import deep_julia_ref as J
import deep_ref as R
import deep_ship_ref as S
import deepx_bla_ref as XB
import deepx_ref as X
from deepx_ref import X_THR, X_ZERO, _ld, _norm

EPS = BR.EPS
E_LIM = XB.E_LIM


def entries(N: int) -> int:
    """(N - 1) - popcount(N - 1): the entries of a table over an orbit Z_0 .. Z_N"""
    return (N - 1) - bin(N - 1).count("1") if N >= 1 else 0


# ---- the tables --------------------------------------------------------------------------------------------------------------
def bla_table(orbit: np.ndarray):
    """Levels 1 .. K of one orbit: a list of dicts (index k - 1) with arrays r, ax, ay over the entries j of the level"""
    N = len(orbit) - 1
    K = BR.levels(N)
    if K == 0:
        return []
    with np.errstate(all="ignore"):
        zx, zy = orbit[1:N, 0].copy(), orbit[1:N, 1].copy()          # the single steps m = 1 .. N - 1
        prev = dict(r=np.float64(EPS) * BR._abs(zx, zy), ax=zx + zx, ay=zy + zy)
        out = []
        for k in range(1, K + 1):
            cnt = (N - 1) >> k
            x = {key: v[0:2 * cnt:2] for key, v in prev.items()}
            y = {key: v[1:2 * cnt:2] for key, v in prev.items()}
            ax = y["ax"] * x["ax"] - y["ay"] * x["ay"]
            ay = y["ax"] * x["ay"] + y["ay"] * x["ax"]
            t = y["r"] / BR._abs(x["ax"], x["ay"])
            r = np.where(t > 0.0, t, 0.0)
            r = np.where(r < x["r"], r, x["r"])
            r = np.where(np.isfinite(ax) & np.isfinite(ay), r, 0.0)
            prev = dict(r=r, ax=ax, ay=ay)
            out.append(prev)
    return out


def bla_tables(P: np.ndarray, Q: np.ndarray):
    """(Q's table, P's table)"""
    return bla_table(Q), bla_table(P)


def bla_table_x(mant: np.ndarray, exp2: np.ndarray):
    """Levels 1 .. K of one extended orbit: dicts with rv, re (the stored radius), ax, ay, ea"""
    N = len(exp2) - 1
    K = BR.levels(N)
    if K == 0:
        return []
    with np.errstate(all="ignore"):
        zx, zy = mant[1:N, 0].copy(), mant[1:N, 1].copy()
        ze = exp2[1:N].astype(np.int64)
        ax, ay, ea = _norm(zx, zy, ze + 1)
        nx, ny, ne = _norm(zx, zy, ze)
        rv, re = XB._abs_x(nx, ny, ne)
        re = np.where(rv == 0.0, X_ZERO, re - 53)
        prev = dict(rv=rv, re=re, ax=ax, ay=ay, ea=ea)
        out = []
        for k in range(1, K + 1):
            cnt = (N - 1) >> k
            x = {key: v[0:2 * cnt:2] for key, v in prev.items()}
            y = {key: v[1:2 * cnt:2] for key, v in prev.items()}
            ax, ay, ea = _norm(y["ax"] * x["ax"] - y["ay"] * x["ay"], y["ax"] * x["ay"] + y["ay"] * x["ax"], y["ea"] + x["ea"])
            av, ae = XB._abs_x(x["ax"], x["ay"], x["ea"])
            t = y["rv"] / av
            ok = (t > 0.0) & np.isfinite(t)
            rv, re = XB._norm1(np.where(ok, t, 0.0), y["re"] - ae)
            less = (re < x["re"]) | ((re == x["re"]) & (rv < x["rv"]))
            rv, re = np.where(less, rv, x["rv"]), np.where(less, re, x["re"])
            void = np.abs(ea) > E_LIM
            rv, re = np.where(void, 0.0, rv), np.where(void, X_ZERO, re)
            ax, ay, ea = np.where(void, 0.0, ax), np.where(void, 0.0, ay), np.where(void, X_ZERO, ea)
            prev = dict(rv=XB._trunc(rv), re=re, ax=ax, ay=ay, ea=ea)
            out.append(prev)
    return out


def bla_tables_x(Px, Qx):
    """(Q's table, P's table) of orbits in the extended storage, each (mant, exp2)"""
    return bla_table_x(Qx[0], Qx[1]), bla_table_x(Px[0], Px[1])


def flat(tabs):
    """(r, a) of a (Q, P) pair in the order of the device buffers: r (n,), a (n, 2)"""
    lv = [T for tab in tabs for T in tab]
    if not lv:
        return np.zeros(0), np.zeros((0, 2))
    return np.concatenate([T["r"] for T in lv]), np.concatenate([np.stack([T["ax"], T["ay"]], axis=1) for T in lv])


def flat_x(tabs):
    """(rv as float32, re, a, ea) of a (Q, P) pair in the order of the device buffers"""
    lv = [T for tab in tabs for T in tab]
    if not lv:
        return np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros(0, np.int32)
    return (np.concatenate([T["rv"] for T in lv]).astype(np.float32), np.concatenate([T["re"] for T in lv]).astype(np.int32),
            np.concatenate([np.stack([T["ax"], T["ay"]], axis=1) for T in lv]), np.concatenate([T["ea"] for T in lv]).astype(np.int32))


def _joined(tabs, keys):
    """Per level (index k - 1) the arrays of Q's level followed by P's, and where P's start: a lane looks its entry up at
    j + (on P ? off : 0)"""
    tq, tp = tabs
    out = []
    for k in range(max(len(tq), len(tp))):
        q = tq[k] if k < len(tq) else None
        p = tp[k] if k < len(tp) else None
        lvl = {key: np.concatenate([(q[key] if q else np.zeros(0, (p or q)[key].dtype)), (p[key] if p else np.zeros(0, (q or p)[key].dtype))])
               for key in keys}
        lvl["off"] = len(q[keys[0]]) if q else 0
        out.append(lvl)
    return out


def _ctz(x: np.ndarray, K: np.ndarray) -> np.ndarray:
    """count of trailing zero bits, K for x == 0"""
    low = x & -x
    out = K.astype(np.int64).copy()
    nz = low > 0
    out[nz] = np.log2(low[nz].astype(np.float64)).astype(np.int64)
    return out


def _top_level(mc, Kc, Nc, max_iter, uc):
    kk = np.minimum(_ctz(mc - 1, Kc), Kc)
    kk = np.minimum(kk, BR._flog2(Nc - mc))
    return np.minimum(kk, BR._flog2(max_iter - uc))


# ---- fp64 stepping -----------------------------------------------------------------------------------------------------------
def perturb_bla(P: np.ndarray, Q: np.ndarray, tabs, d0x: np.ndarray, d0y: np.ndarray, max_iter: int, bailout: float = 4.0):
    """deep_julia_ref.perturb with BLA.  Returns (iter, r2, counts, on): counts = [plain steps, BLA steps, updates skipped],
    on = [BLA steps on Q, BLA steps on P]."""
    ox = np.concatenate([Q[:, 0], P[:, 0]])
    oy = np.concatenate([Q[:, 1], P[:, 1]])
    NQ, NP, poff = len(Q) - 1, len(P) - 1, len(Q)
    KQ, KP = len(tabs[0]), len(tabs[1])
    T = _joined(tabs, ("r", "ax", "ay"))
    B2 = np.float64(np.float32(bailout)) * np.float64(np.float32(bailout))
    shape = d0x.shape
    dzx, dzy = d0x.ravel().astype(np.float64).copy(), d0y.ravel().astype(np.float64).copy()
    n = dzx.size
    it = np.full(n, max_iter, np.int32)
    r2out = np.zeros(n, np.float64)
    idx = np.arange(n)
    m = np.zeros(n, np.int64)
    u = np.zeros(n, np.int64)
    onp = np.ones(n, bool)                                          # on P: its base, N, K and table
    counts, on = [0, 0, 0], [0, 0]
    while idx.size:
        base = np.where(onp, poff, 0)
        N = np.where(onp, NP, NQ)
        Kl = np.where(onp, KP, KQ)
        Zx, Zy = ox[base + m], oy[base + m]
        dz2 = dzx * dzx + dzy * dzy
        k = np.zeros(idx.size, np.int64)
        r0 = np.float64(EPS) * BR._abs(Zx, Zy)                      # no level's r exceeds the single step's
        cand = np.nonzero((m >= 1) & (dz2 < r0 * r0) & (Kl > 0))[0]
        if cand.size:
            mc, pc = m[cand], onp[cand]
            kk = _top_level(mc, Kl[cand], N[cand], max_iter, u[cand])
            for lvl in range(len(T), 0, -1):                          # top down: the largest valid k
                sel = np.nonzero(kk == lvl)[0]
                if sel.size == 0:
                    continue
                r = T[lvl - 1]["r"][((mc[sel] - 1) >> lvl) + np.where(pc[sel], T[lvl - 1]["off"], 0)]
                bad = ~(dz2[cand[sel]] < r * r)
                kk[sel[bad]] -= 1
            k[cand] = np.maximum(kk, 0)
        bl = k > 0
        tx = (Zx + Zx) + dzx
        ty = (Zy + Zy) + dzy
        nx = tx * dzx - ty * dzy
        ny = tx * dzy + ty * dzx
        if bl.any():
            b = np.nonzero(bl)[0]
            kb = k[b]
            ax = np.empty(b.size); ay = np.empty(b.size)
            for lvl in np.unique(kb):
                s = kb == lvl
                j = ((m[b[s]] - 1) >> lvl) + np.where(onp[b[s]], T[lvl - 1]["off"], 0)
                ax[s], ay[s] = T[lvl - 1]["ax"][j], T[lvl - 1]["ay"][j]
            ex, ey = dzx[b], dzy[b]
            nx[b] = ax * ex - ay * ey
            ny[b] = ax * ey + ay * ex
        step = np.where(bl, np.left_shift(1, k), 1)
        counts[0] += int((~bl).sum())
        counts[1] += int(bl.sum())
        counts[2] += int(step[bl].sum())
        on[0] += int((bl & ~onp).sum())
        on[1] += int((bl & onp).sum())
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
        keep = ~esc & (u < max_iter)
        if not keep.all():
            idx, dzx, dzy, m, u, onp = idx[keep], dzx[keep], dzy[keep], m[keep], u[keep], onp[keep]
    return it.reshape(shape), r2out.reshape(shape), counts, on


def restate_bla(v: dict, W: int, H: int, aa: int = 1, bailout: float = 4.0, rows=None, orbits=None, tabs=None, stats=None):
    """Every sub-sample of the frame (or of its rows): a list over s of (iter, r2) planes, and the three counts summed.
    stats (a dict) receives bla_q / bla_p, the BLA steps taken on each orbit."""
    P, Q = orbits if orbits is not None else J.reference_orbits(v, bailout)
    if tabs is None:
        tabs = bla_tables(P, Q)
    out, total = [], [0, 0, 0]
    for s in range(aa * aa):
        d0x, d0y = S.sample_dc(W, H, v["zoom"], aa, s, rows)
        it, r2, c, on = perturb_bla(P, Q, tabs, d0x, d0y, v["max_iter"], bailout)
        out.append((it, r2))
        total = [a + b for a, b in zip(total, c)]
        if stats is not None:
            stats["bla_q"] = stats.get("bla_q", 0) + on[0]
            stats["bla_p"] = stats.get("bla_p", 0) + on[1]
    return out, total


# ---- extended stepping -------------------------------------------------------------------------------------------------------
def perturb_x_bla(Px, Qx, tabs, d0, max_iter: int, bailout: float = 4.0):
    """deep_julia_ref.perturb_x with BLA steps in both modes.  Returns (iter, r2, counts, on) as perturb_bla."""
    mant = np.concatenate([Qx[0], Px[0]])
    exp2 = np.concatenate([Qx[1], Px[1]])
    omx, omy = np.ascontiguousarray(mant[:, 0]), np.ascontiguousarray(mant[:, 1])
    oe = exp2.astype(np.int64)
    plain = X.decode(mant, exp2)
    opx, opy = np.ascontiguousarray(plain[:, 0]), np.ascontiguousarray(plain[:, 1])
    NQ, NP, poff = len(Qx[1]) - 1, len(Px[1]) - 1, len(Qx[1])
    KQ, KP = len(tabs[0]), len(tabs[1])
    T = _joined(tabs, ("rv", "re", "ax", "ay", "ea"))
    B2 = np.float64(np.float32(bailout)) * np.float64(np.float32(bailout))
    x0, y0, e0 = d0
    n = x0.size
    it = np.full(n, max_iter, np.int32)
    r2out = np.zeros(n, np.float64)
    idx = np.arange(n)
    ext = e0 <= X_THR                                               # the mode rule, applied at once
    with np.errstate(all="ignore"):
        dx = np.where(ext, x0, _ld(x0, np.where(ext, 0, e0)))
        dy = np.where(ext, y0, _ld(y0, np.where(ext, 0, e0)))
    ed = e0.astype(np.int64).copy()
    m = np.zeros(n, np.int64)
    u = np.zeros(n, np.int64)
    onp = np.ones(n, bool)
    counts, on = [0, 0, 0], [0, 0]

    def finish(Sx, bb, NN, mm, nx, ny, en, esc, r2e):
        """z = Z_m (+) n, the escape test, the two-orbit rebase rule, norm, the flush and the mode rule, for the samples Sx"""
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
        fl = ea < J.X_FLUSH
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
            was_p = onp.copy()
            esc = np.zeros(idx.size, bool)
            r2e = np.zeros(idx.size)
            k = np.zeros(idx.size, np.int64)
            cand = np.nonzero((m >= 1) & (Kl > 0))[0]
            if cand.size:
                # dz as a normalised extended number: an extended lane has it, a plain lane forms norm(dz.x, dz.y, 0)
                qx, qy, qe = _norm(dx[cand], dy[cand], np.zeros(cand.size, np.int64))
                isx = ext[cand]
                qx, qy, qe = np.where(isx, dx[cand], qx), np.where(isx, dy[cand], qy), np.where(isx, ed[cand], qe)
                dz2 = qx * qx + qy * qy
                mc, pc = m[cand], onp[cand]
                kk = _top_level(mc, Kl[cand], N[cand], max_iter, u[cand])
                for lvl in range(len(T), 0, -1):                      # top down: the largest valid k
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
                        s = kb == lvl
                        j = ((mc[b[s]] - 1) >> lvl) + np.where(pc[b[s]], T[lvl - 1]["off"], 0)
                        ax[s], ay[s], ea[s] = T[lvl - 1]["ax"][j], T[lvl - 1]["ay"][j], T[lvl - 1]["ea"][j]
                    x, y, e = qx[b], qy[b], qe[b]
                    finish(Bl, base[Bl], N[Bl], mc[b] + np.left_shift(1, kb), ax * x - ay * y, ax * y + ay * x, ea + e, esc, r2e)
            bl = k > 0
            E = np.nonzero(ext & ~bl)[0]
            Pl = np.nonzero(~ext & ~bl)[0]
            # a BLA step may have changed ext of its own lanes: E and Pl are the single-step lanes, which no BLA step touched
            if E.size:
                mm, bb = m[E], base[E]
                Zx, Zy, eZ = omx[bb + mm], omy[bb + mm], oe[bb + mm]
                x, y, e = dx[E], dy[E], ed[E]
                et = np.maximum(eZ + 1, e)
                tx = _ld(Zx, eZ + 1 - et) + _ld(x, e - et)
                ty = _ld(Zy, eZ + 1 - et) + _ld(y, e - et)
                finish(E, bb, N[E], mm + 1, tx * x - ty * y, tx * y + ty * x, et + e, esc, r2e)
            if Pl.size:
                mm, bb = m[Pl], base[Pl]
                Zx, Zy = opx[bb + mm], opy[bb + mm]
                x, y = dx[Pl], dy[Pl]
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
            on[0] += int((bl & ~was_p).sum())
            on[1] += int((bl & was_p).sum())
            u = u + step
            it[idx[esc]] = (u[esc] - 1).astype(np.int32)
            r2out[idx[esc]] = r2e[esc]
            keep = ~esc & (u < max_iter)
            if not keep.all():
                idx, dx, dy, ed, ext, m, u, onp = idx[keep], dx[keep], dy[keep], ed[keep], ext[keep], m[keep], u[keep], onp[keep]
    return it, r2out, counts, on


def restate_x_bla(v: dict, W: int, H: int, aa: int = 1, bailout: float = 4.0, rows=None, orbits=None, tabs=None, stats=None):
    """restate_bla through the extended restatement (the view's zoom_s)"""
    Px, Qx = orbits if orbits is not None else J.reference_orbits_x(v, bailout)
    if tabs is None:
        tabs = bla_tables_x(Px, Qx)
    zm, ze = X.zoom_pair(v["zoom_s"])
    nrows = H if rows is None else len(rows)
    out, total = [], [0, 0, 0]
    for s in range(aa * aa):
        it, r2, c, on = perturb_x_bla(Px, Qx, tabs, J.sample_d0_x(W, H, zm, ze, aa, s, rows), v["max_iter"], bailout)
        out.append((it.reshape(nrows, W), r2.reshape(nrows, W)))
        total = [a + b for a, b in zip(total, c)]
        if stats is not None:
            stats["bla_q"] = stats.get("bla_q", 0) + on[0]
            stats["bla_p"] = stats.get("bla_p", 0) + on[1]
    return out, total


# ---- a centre on a pre-critical point -------------------------------------------------------------------------------------------
def precritical_centre(c, depth: int, D: int):
    """A depth-`depth` preimage of 0 under z^2 + c: w_0 = 0, w_{i+1} = sqrt(w_i - c), always the root with re >= 0 (im >= 0
    where re == 0), at 200 + D digits, quantised to D decimals: (cx, cy) strings.  c = (re, im) doubles, taken exactly."""
    with decimal.localcontext() as ctx:
        ctx.prec = 200 + D
        Dm = decimal.Decimal
        cr, ci = Dm(c[0]), Dm(c[1])
        wr, wi = Dm(0), Dm(0)
        for _ in range(depth):
            a, b = wr - cr, wi - ci
            r = (a * a + b * b).sqrt()
            re = ((r + a) / 2).sqrt()
            im = ((r - a) / 2).sqrt()
            if b < 0:
                im = -im
            wr, wi = re, im
        q = Dm(1).scaleb(-D)
        x = wr.quantize(q, rounding=decimal.ROUND_HALF_EVEN)
        y = wi.quantize(q, rounding=decimal.ROUND_HALF_EVEN)
        return ("0" if x == 0 else format(x, "f")), ("0" if y == 0 else format(y, "f"))


PRECRIT_DEPTH, PRECRIT_DIGITS = 12, 61


@functools.lru_cache(maxsize=None)
def _precrit60():
    cx, cy = precritical_centre((0.0, 1.0), PRECRIT_DEPTH, PRECRIT_DIGITS)
    return dict(name="PRECRIT60", c=(0.0, 1.0), cx=cx, cy=cy, zoom=1e-60, zoom_s="1e-60", max_iter=1000, F=R.frac_bits(1e-60))


def view(name: str) -> dict:
    """deep_julia_ref's views and PRECRIT60: the dendrite (c = i) at 1e-60 around a depth-12 preimage of 0 quantised to 61
    decimals, so that the preimage itself lies inside the view, a fraction of a view height off the centre.  P_12 is then of
    the size of the deltas: the samples nearer to the preimage than to the centre rebase there (|z| < |dz|), square their
    delta on Q's first step and follow Q from about 2^-400 upwards, inside the radii of Q's table; the others stay on P.  (A
    centre quantised much finer has P_12 below every delta's last bit, z = dz' in fp64, and no sample ever rebases: measured
    with 90 decimals, 0 BLA steps on Q.)  Depth 12 and 61 decimals were chosen on the CPU from depths 6, 12, 20 and 60 .. 62
    decimals (15493 .. 36514 BLA steps on Q at 128 x 96): 35699 here."""
    return _precrit60() if name == "PRECRIT60" else J.view(name)


# ---- what the tests share: computed once per session, never changed ---------------------------------------------------------
BW, BH = 128, 96


@functools.lru_cache(maxsize=None)
def orbits(name: str):
    return J.reference_orbits(view(name))


@functools.lru_cache(maxsize=None)
def orbits_x(name: str):
    return J.reference_orbits_x(view(name))


@functools.lru_cache(maxsize=None)
def restated_bla(name: str, aa: int = 1, W: int = BW, H: int = BH):
    """(samples, counts, stats) of the flagged fp64 restatement"""
    stats = {}
    out, counts = restate_bla(view(name), W, H, aa, orbits=orbits(name), stats=stats)
    return out, counts, stats


@functools.lru_cache(maxsize=None)
def restated_x_bla(name: str, aa: int = 1, W: int = BW, H: int = BH):
    stats = {}
    out, counts = restate_x_bla(view(name), W, H, aa, orbits=orbits_x(name), stats=stats)
    return out, counts, stats


@functools.lru_cache(maxsize=None)
def unflagged(name: str, W: int = BW, H: int = BH):
    return J.restate(view(name), W, H, orbits=orbits(name))[0][0]


@functools.lru_cache(maxsize=None)
def unflagged_x(name: str, W: int = BW, H: int = BH):
    return J.restate_x(view(name), W, H, orbits=orbits_x(name))[0][0]
