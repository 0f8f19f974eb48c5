"""Deep Phoenix views below 1e-290 with bilinear approximation (fr_render_deepx_phoenix with FR_FLAG_DEEPX_PHOENIX_BLA): the table
build and the stepping of the header, restated operation for operation in numpy, vectorised over samples.  TEST INFRASTRUCTURE
ONLY.

It is deep_phoenix_bla_ref's scheme -- a complex 2 x 2 matrix M, a complex 2-vector B and a radius on the pair (dz, dq) -- in the
extended arithmetic of deepx_bla_ref / deepx_ship_bla_ref: M's eight mantissas share one exponent, B's four another, the radius
is a 24-bit mantissa and an exponent.

- single_steps_x / bla_table_x: the single steps (never stored) and the levels k = 1 .. K, as the device builds them;
- table_arrays: the table as fr_deepx_phoenix_bla_table reads it back;
- perturb_x_bla: deepx_phoenix_ref.perturb_x's two-mode step with BLA steps in both modes; (iter, lastZ) and the three counts;
- samples_x_bla / restate_x_bla: every sub-sample of a frame, the counts summed (fr_ctx_last_deepx_phoenix_steps), the planes.

deepx_phoenix_ref.py supplies the orbit and the views, deepx_ref.py the extended arithmetic, deep_phoenix_ref.py the colour stage.
"""
from __future__ import annotations

import numpy as np

import deep_bla_ref as BR
import deep_phoenix_ref as P
import deepx_phoenix_ref as PX
import deepx_ref as X
import deepx_ship_ref as SX
from deep_phoenix_bla_ref import ELEMS, ENTRY_DOUBLES, _cadd, _cmul, _n2
from deepx_bla_ref import E_LIM, _norm1, _trunc
from deepx_ref import X_THR, X_ZERO, _THR, _ld, _norm
from deepx_ship_bla_ref import _less, dcmax_ship_x

F32 = np.float32
M_ELEMS, B_ELEMS = ELEMS[:4], ELEMS[4:]

# the period-201 nucleus of deepx_views.json at 1e-1000, p = r = 0: the orbit returns to 2^-1312 once per period, where a radius
# formed in a double underflows; 12 periods
NUC201X = dict(cx=X.views()["nucleus201"]["cx"], cy=X.views()["nucleus201"]["cy"], zoom="1e-1000", max_iter=2412, p=0.0, r=0.0)
VIEWS = dict(PX.NEW_VIEWS, NUC201X=NUC201X)


def _normc(cs, e):
    """norm of the header on a list of complex mantissas (pairs of arrays) sharing the exponent e: the largest of all components
    into [0.5, 1); all zero gets X_ZERO"""
    mx = np.zeros_like(cs[0][0])
    for c in cs:
        mx = np.maximum(mx, np.maximum(np.abs(c[0]), np.abs(c[1])))
    _, k = np.frexp(mx)
    k = k.astype(np.int64)
    return [(_ld(c[0], -k), _ld(c[1], -k)) for c in cs], np.where(mx == 0.0, X_ZERO, e + k)


def _xadd(a, ea, b, eb):
    """(a, ea) (+) (b, eb) per component at e = max(ea, eb): (sum, e)"""
    e = np.maximum(ea, eb)
    return (_ld(a[0], ea - e) + _ld(b[0], eb - e), _ld(a[1], ea - e) + _ld(b[1], eb - e)), e


def _term_exp(t, e):
    """the exponent of a BLA step's term: X_ZERO for a term that is exactly zero"""
    return np.where((t[0] == 0.0) & (t[1] == 0.0), X_ZERO, e)


def single_steps_x(mant: np.ndarray, exp2: np.ndarray, p: float, r: float, double_radius: bool = False) -> dict:
    """The single steps m = 1 .. N - 1: a = (Z, eZ + 1) (+) (p, pe); M = norm(a, (r, 0), (1, 0), 0) on the common exponent
    max(a.e, 0); B = norm((1, 0), 0); rad = 2^-54 |norm(a)|, the factor in the exponent.  double_radius: the radius rounded
    through a double (what the table must NOT do: the measurement of test_deepx_phoenix_bla_host.py)."""
    N = len(exp2) - 1
    Xm, Ym = mant[1:N, 0].copy(), mant[1:N, 1].copy()
    eZ = exp2[1:N].astype(np.int64)
    p, r = np.float64(F32(p)), np.float64(F32(r))
    pe = X_ZERO if p == 0.0 else 0
    ea = np.maximum(eZ + 1, pe)
    ax = _ld(Xm, eZ + 1 - ea) + _ld(np.full(Xm.size, p), pe - ea)
    ay = _ld(Ym, eZ + 1 - ea)
    em = np.maximum(ea, 0)
    one, zero = np.ones_like(Xm), np.zeros_like(Xm)
    M, em = _normc([(_ld(ax, ea - em), _ld(ay, ea - em)), (_ld(zero + r, -em), zero), (_ld(one, -em), zero), (zero, zero)], em)
    B, eb = _normc([(one, zero), (zero, zero)], np.zeros_like(eZ))
    nx, ny, ne = _norm(ax, ay, ea)
    rv, re = _norm1(np.sqrt(nx * nx + ny * ny), ne)
    re = np.where(rv == 0.0, X_ZERO, re - 54)
    if double_radius:
        rv, re = _norm1(_ld(rv, re), np.zeros_like(re))
    out = dict(rv=rv, re=re, em=em, eb=eb)
    out.update(zip(M_ELEMS, M))
    out.update(zip(B_ELEMS, B))
    return out


def bla_table_x(mant: np.ndarray, exp2: np.ndarray, dcm, p: float, r: float, double_radius: bool = False):
    """Levels 1 .. K: a list of dicts (index k - 1) with arrays rv, re (the stored radius), the six complex mantissas of ELEMS
    (pairs of arrays), em and eb over the entries j of the level, entry j covering the 2^k steps from m = 1 + j * 2^k"""
    N = len(exp2) - 1
    K = BR.levels(N)
    if K == 0:
        return []
    dv, de = np.float64(dcm[0]), np.int64(dcm[1])
    with np.errstate(all="ignore"):
        prev = single_steps_x(mant, exp2, p, r, double_radius)
        out = []
        for k in range(1, K + 1):
            cnt = (N - 1) >> k
            half = lambda v, o: v[o:2 * cnt:2] if isinstance(v, np.ndarray) else (v[0][o:2 * cnt:2], v[1][o:2 * cnt:2])
            x = {q: half(v, 0) for q, v in prev.items()}
            y = {q: half(v, 1) for q, v in prev.items()}
            m, q = {}, []
            for i in ("1", "2"):
                for j in ("1", "2"):
                    m["m" + i + j] = _cadd(_cmul(y["m" + i + "1"], x["m1" + j]), _cmul(y["m" + i + "2"], x["m2" + j]))
                q.append(_cadd(_cmul(y["m" + i + "1"], x["b1"]), _cmul(y["m" + i + "2"], x["b2"])))
            M, em = _normc([m[e] for e in M_ELEMS], y["em"] + x["em"])
            e1 = y["em"] + x["eb"]
            eb = np.maximum(e1, y["eb"])
            B, eb = _normc([(_ld(q[i][0], e1 - eb) + _ld(y[b][0], y["eb"] - eb), _ld(q[i][1], e1 - eb) + _ld(y[b][1], y["eb"] - eb))
                            for i, b in enumerate(B_ELEMS)], eb)
            av, ae = _norm1(np.sqrt((_n2(x["m11"]) + _n2(x["m12"])) + (_n2(x["m21"]) + _n2(x["m22"]))), x["em"])
            bv, be = _norm1(np.sqrt(_n2(x["b1"]) + _n2(x["b2"])), x["eb"])
            pv, pe = bv * dv, be + de
            et = np.maximum(y["re"], pe)
            num = _ld(y["rv"], y["re"] - et) - _ld(pv, pe - et)
            t = num / av
            ok = (t > 0.0) & np.isfinite(t)
            rv, re = _norm1(np.where(ok, t, 0.0), et - ae)
            keep_x = (av == 0.0) & (num > 0.0)                       # M_x is the zero matrix: t = +inf, rad = rad_x
            less = _less(rv, re, x["rv"], x["re"]) & ~keep_x
            rv, re = np.where(less, rv, x["rv"]), np.where(less, re, x["re"])
            void = ((np.abs(em) > E_LIM) & (em != X_ZERO)) | (np.abs(eb) > E_LIM)
            rv, re = np.where(void, 0.0, rv), np.where(void, X_ZERO, re)
            prev = dict(rv=_trunc(rv), re=re, em=np.where(void, X_ZERO, em), eb=np.where(void, X_ZERO, eb))
            prev.update((n, (np.where(void, 0.0, c[0]), np.where(void, 0.0, c[1]))) for n, c in zip(M_ELEMS, M))
            prev.update((n, (np.where(void, 0.0, c[0]), np.where(void, 0.0, c[1]))) for n, c in zip(B_ELEMS, B))
            out.append(prev)
    return out


def table_arrays(table):
    """The table as fr_deepx_phoenix_bla_table reads it back: (n, 2) uint32 words of the radius (the float's bits, the int32
    exponent's), (n, 12) mantissas M11, M12, M21, M22, B1, B2, and (n, 2) int32 exponents (M.e, B.e)"""
    rv = np.concatenate([T["rv"] for T in table]).astype(np.float32)
    re = np.concatenate([T["re"] for T in table]).astype(np.int32)
    r = np.stack([rv.view(np.uint32), re.view(np.uint32)], axis=1)
    mb = np.concatenate([np.stack([T[q][c] for q in ELEMS for c in (0, 1)], axis=1) for T in table])
    ex = np.concatenate([np.stack([T["em"], T["eb"]], axis=1) for T in table]).astype(np.int32)
    return r, mb, ex


def perturb_x_bla(mant, exp2, dc, max_iter: int, p: float, r: float, table):
    """The two-mode step of the header with BLA on flat sample arrays.  Returns (iter, lastZ x, lastZ y, counts): counts =
    [single steps of both modes, BLA steps, updates skipped] over the samples."""
    omx, omy = np.ascontiguousarray(mant[:, 0]), np.ascontiguousarray(mant[:, 1])
    oe = exp2.astype(np.int64)
    plain = X.decode(mant, exp2)
    opx, opy = np.ascontiguousarray(plain[:, 0]), np.ascontiguousarray(plain[:, 1])
    N = len(oe) - 1
    K = len(table)
    p, r = np.float64(F32(p)), np.float64(F32(r))
    rr = r * r
    pe = X_ZERO if p == 0.0 else 0
    four = np.float64(4.0)
    cx, cy, ec, cpx, cpy = dc
    n = cx.size
    it = np.full(n, max_iter, np.int32)
    ezx = np.zeros(n); ezy = np.zeros(n)
    idx = np.arange(n)
    dx = np.zeros(n); dy = np.zeros(n); qx_ = np.zeros(n); qy_ = np.zeros(n)
    ed = np.full(n, X_ZERO, np.int64); eq = np.full(n, X_ZERO, np.int64)
    ext = np.ones(n, bool)
    m = np.zeros(n, np.int64)
    u = np.zeros(n, np.int64)
    counts = [0, 0, 0]

    def finish(S, mm, nz, en, nq, enq, Pm, eP, bla, esc, lzx, lzy):
        """the EXTENDED step's tail for the samples S at their new m = mm: z = Z_m (+) dz', q = Z_{m-1} (+) dq', the escape test,
        the pair rebase rule with its four terms at z's exponent, norm and the mode rule.  bla: dq is normalised where it is
        stored (a BLA step's dq' is computed); else it is the copy, or (q, eq') with X_ZERO for q = 0."""
        nx, ny = nz
        nqx, nqy = nq
        Wx, Wy, eW = omx[mm], omy[mm], oe[mm]
        ez = np.maximum(eW, en)
        zx = _ld(Wx, eW - ez) + _ld(nx, en - ez)
        zy = _ld(Wy, eW - ez) + _ld(ny, en - ez)
        eqq = np.maximum(eP, enq)
        qx = _ld(Pm[0], eP - eqq) + _ld(nqx, enq - eqq)
        qy = _ld(Pm[1], eP - eqq) + _ld(nqy, enq - eqq)
        r2 = zx * zx + zy * zy
        es = _ld(r2, 2 * ez) > four
        lhs = r2 + _ld(rr * (qx * qx + qy * qy), 2 * (eqq - ez))
        rhs = _ld(nx * nx + ny * ny, 2 * (en - ez)) + _ld(rr * (nqx * nqx + nqy * nqy), 2 * (enq - ez))
        reb = ~es & ((lhs < rhs) | (mm == N))
        ax, ay, ea = _norm(np.where(reb, zx, nx), np.where(reb, zy, ny), np.where(reb, ez, en))
        gx = np.where(reb, qx, nqx); gy = np.where(reb, qy, nqy)
        ge = np.where(reb, np.where((qx == 0.0) & (qy == 0.0), X_ZERO, eqq), enq)
        if bla:
            gx, gy, ge = _norm(gx, gy, ge)
        stay = ea <= X_THR
        dx[S] = np.where(stay, ax, _ld(ax, np.where(stay, 0, ea)))
        dy[S] = np.where(stay, ay, _ld(ay, np.where(stay, 0, ea)))
        ed[S] = ea
        qx_[S] = np.where(stay, gx, _ld(gx, np.where(stay, 0, ge)))
        qy_[S] = np.where(stay, gy, _ld(gy, np.where(stay, 0, ge)))
        eq[S] = ge
        ext[S] = stay
        m[S] = np.where(reb, 0, mm)
        esc[S] = es
        lzx[S] = _ld(zx, ez); lzy[S] = _ld(zy, ez)

    with np.errstate(all="ignore"):
        while idx.size:
            esc = np.zeros(idx.size, bool)
            lzx = np.zeros(idx.size); lzy = np.zeros(idx.size)
            k = np.zeros(idx.size, np.int64)
            cand = np.nonzero(m >= 1)[0] if K else np.zeros(0, np.int64)
            if cand.size:
                # the pair as two normalised extended numbers: an extended lane has them, a plain lane forms norm(dz, 0), norm(dq, 0)
                zero = np.zeros(cand.size, np.int64)
                isx = ext[cand]
                vzx, vzy, vze = _norm(dx[cand], dy[cand], zero)
                vqx, vqy, vqe = _norm(qx_[cand], qy_[cand], zero)
                vzx, vzy, vze = np.where(isx, dx[cand], vzx), np.where(isx, dy[cand], vzy), np.where(isx, ed[cand], vze)
                vqx, vqy, vqe = np.where(isx, qx_[cand], vqx), np.where(isx, qy_[cand], vqy), np.where(isx, eq[cand], vqe)
                ev = np.maximum(vze, vqe)
                a, b = _ld(vzx, vze - ev), _ld(vzy, vze - ev)
                c, d = _ld(vqx, vqe - ev), _ld(vqy, vqe - ev)
                v2 = (a * a + b * b) + (c * c + d * d)
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
                    bad = ~(v2[sel] < _ld(rv * rv, 2 * (re - ev[sel])))
                    kk[sel[bad]] -= 1
                kk = np.maximum(kk, 0)
                k[cand] = kk
                b_ = np.nonzero(kk > 0)[0]
                if b_.size:
                    Bl = cand[b_]
                    kb = kk[b_]
                    j = (mc[b_] - 1) >> kb
                    E = {q: (np.empty(b_.size), np.empty(b_.size)) for q in ELEMS}
                    em = np.empty(b_.size, np.int64); eb = np.empty(b_.size, np.int64)
                    for lvl in np.unique(kb):
                        s = kb == lvl
                        T = table[lvl - 1]
                        for q in ELEMS:
                            E[q][0][s] = T[q][0][j[s]]
                            E[q][1][s] = T[q][1][j[s]]
                        em[s], eb[s] = T["em"][j[s]], T["eb"][j[s]]
                    dz, dq, dcc = (vzx[b_], vzy[b_]), (vqx[b_], vqy[b_]), (cx[Bl], cy[Bl])
                    e_z, e_q, e_c = em + vze[b_], em + vqe[b_], eb + ec[Bl]
                    new = []
                    for row in (("m11", "m12", "b1"), ("m21", "m22", "b2")):
                        t1, t2, t3 = _cmul(E[row[0]], dz), _cmul(E[row[1]], dq), _cmul(E[row[2]], dcc)
                        t12, e12 = _xadd(t1, _term_exp(t1, e_z), t2, _term_exp(t2, e_q))
                        new.append(_xadd(t12, e12, t3, _term_exp(t3, e_c)))
                    mm = mc[b_] + np.left_shift(1, kb)
                    finish(Bl, mm, new[0][0], new[0][1], new[1][0], new[1][1], (omx[mm - 1], omy[mm - 1]), oe[mm - 1], True,
                           esc, lzx, lzy)
            bl = k > 0
            # the single-step lanes in the mode they had BEFORE this trip: a BLA step may have changed ext of its own lanes
            Es = np.nonzero(ext & ~bl)[0]
            Q = np.nonzero(~ext & ~bl)[0]
            if Es.size:
                mm = m[Es]
                Zx, Zy, eZ = omx[mm], omy[mm], oe[mm]
                a, b, e = dx[Es], dy[Es], ed[Es]
                c, d, f = qx_[Es], qy_[Es], eq[Es]
                eu = np.maximum(eZ + 1, e)
                ux = _ld(Zx, eZ + 1 - eu) + _ld(a, e - eu)
                uy = _ld(Zy, eZ + 1 - eu) + _ld(b, e - eu)
                et = np.maximum(eu, pe)
                tx = _ld(ux, eu - et) + _ld(np.full(Es.size, p), pe - et)
                ty = _ld(uy, eu - et)
                px = tx * a - ty * b
                py = tx * b + ty * a
                ep = et + e
                er = np.full(Es.size, X_ZERO, np.int64) if r == 0.0 else f
                e1 = np.maximum(ep, er)
                sx = _ld(px, ep - e1) + _ld(r * c, er - e1)
                sy = _ld(py, ep - e1) + _ld(r * d, er - e1)
                en = np.maximum(e1, ec[Es])
                nx = _ld(sx, e1 - en) + _ld(cx[Es], ec[Es] - en)
                ny = _ld(sy, e1 - en) + _ld(cy[Es], ec[Es] - en)
                finish(Es, mm + 1, (nx, ny), en, (a, b), e, (Zx, Zy), eZ, False, esc, lzx, lzy)
            if Q.size:
                mm = m[Q]
                Zx, Zy = opx[mm], opy[mm]
                a, b, c, d = dx[Q], dy[Q], qx_[Q], qy_[Q]
                tx = ((Zx + Zx) + a) + p
                ty = (Zy + Zy) + b
                nx = ((tx * a - ty * b) + r * c) + cpx[Q]
                ny = ((tx * b + ty * a) + r * d) + cpy[Q]
                mm = mm + 1
                zx, zy = opx[mm] + nx, opy[mm] + ny
                qx, qy = Zx + a, Zy + b
                r2 = zx * zx + zy * zy
                es = r2 > four
                small_pair = (r2 + rr * (qx * qx + qy * qy)) < ((nx * nx + ny * ny) + rr * (a * a + b * b))
                reb = ~es & (small_pair | (mm == N))
                ax = np.where(reb, zx, nx); ay = np.where(reb, zy, ny)
                nqx = np.where(reb, qx, a); nqy = np.where(reb, qy, b)
                small = np.maximum(np.abs(ax), np.abs(ay)) < _THR
                bx, by, be = _norm(ax, ay, np.zeros(Q.size, np.int64))
                gx, gy, ge = _norm(nqx, nqy, np.zeros(Q.size, np.int64))
                dx[Q] = np.where(small, bx, ax); dy[Q] = np.where(small, by, ay)
                ed[Q] = be
                qx_[Q] = np.where(small, gx, nqx); qy_[Q] = np.where(small, gy, nqy)
                eq[Q] = ge
                ext[Q] = small
                m[Q] = np.where(reb, 0, mm)
                esc[Q] = es
                lzx[Q] = zx; lzy[Q] = zy
            step = np.where(bl, np.left_shift(1, k), 1)
            counts[0] += int((~bl).sum())
            counts[1] += int(bl.sum())
            counts[2] += int(step[bl].sum())
            u = u + step
            e_ = idx[esc]
            it[e_] = (u[esc] - 1).astype(np.int32)
            ezx[e_] = lzx[esc]; ezy[e_] = lzy[esc]
            done = ~esc & (u >= max_iter)                             # lastZ of a sample that never escaped: Z_m (+) dz
            if done.any():
                md = m[done]
                eZ = oe[md]
                ez = np.maximum(eZ, ed[done])
                lx = _ld(_ld(omx[md], eZ - ez) + _ld(dx[done], ed[done] - ez), ez)
                ly = _ld(_ld(omy[md], eZ - ez) + _ld(dy[done], ed[done] - ez), ez)
                ezx[idx[done]] = np.where(ext[done], lx, opx[md] + dx[done])
                ezy[idx[done]] = np.where(ext[done], ly, opy[md] + dy[done])
            keep = ~esc & ~done
            if not keep.all():
                idx, dx, dy, ed, qx_, qy_, eq, ext, m, u = (v[keep] for v in (idx, dx, dy, ed, qx_, qy_, eq, ext, m, u))
                cx, cy, ec, cpx, cpy = cx[keep], cy[keep], ec[keep], cpx[keep], cpy[keep]
    return it, ezx, ezy, counts


def view_table(view: dict, W: int, H: int, orbit=None, double_radius: bool = False):
    """The table of a view's frame; dcmax is that of the whole W x H frame (the ship's formula on the zoom pair)"""
    mant, exp2 = orbit if orbit is not None else PX.orbit_of(view)
    zm, ze = X.zoom_pair(view["zoom"])
    return bla_table_x(mant, exp2, dcmax_ship_x(W, H, zm, ze), view["p"], view["r"], double_radius)


def samples_x_bla(view: dict, W: int, H: int, aa: int = 1, rows=None, orbit=None, table=None, double_radius: bool = False):
    """Every sub-sample of the frame (or of its rows), sx outer: a list over s of (iter, r2, lastZ x, lastZ y) planes in
    deepx_phoenix_ref.samples_x's layout, and the three counts summed.  dcmax is that of the whole W x H frame, whatever the rows."""
    mant, exp2 = orbit if orbit is not None else PX.orbit_of(view)
    if table is None:
        table = view_table(view, W, H, (mant, exp2), double_radius)
    zm, ze = X.zoom_pair(view["zoom"])
    nrows = H if rows is None else len(rows)
    n_aa = max(int(aa), 1)
    ns = n_aa * n_aa
    dcs = [SX.sample_dc_ship_x(W, H, zm, ze, n_aa, s, rows) for s in range(ns)]
    dc = tuple(np.concatenate([d[k] for d in dcs]) for k in range(5))     # the samples are independent: one pass over all of them
    it, ezx, ezy, counts = perturb_x_bla(mant, exp2, dc, view["max_iter"], view["p"], view["r"], table)
    r2 = np.where(it < view["max_iter"], ezx * ezx + ezy * ezy, 0.0)
    return [tuple(a.reshape(ns, nrows, W)[s] for a in (it, r2, ezx, ezy)) for s in range(ns)], counts


def restate_x_bla(view: dict, W: int, H: int, aa: int = 1, density: float = 0.0, post: bool = False, rows=None, orbit=None,
                  table=None):
    """A frame (or its rows): (iter, nu, rgb, counts) -- iter / nu of sample (0,0), rgb of all of them, the colour stage being
    deep_phoenix_ref's"""
    smp, counts = samples_x_bla(view, W, H, aa, rows, orbit, table)
    it, _, ezx, ezy = smp[0]
    return it, P.smooth(it, ezx, ezy, view["max_iter"]), P.colour(smp, view["max_iter"], density, post), counts
