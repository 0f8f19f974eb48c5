"""Deep Phoenix views with bilinear approximation (fr_render_deep_phoenix with FR_FLAG_DEEP_PHOENIX_BLA): the table build and the
stepping of the header, restated operation for operation in fp64 numpy, vectorised over samples.  TEST INFRASTRUCTURE ONLY.

The recurrence is second order, so the linear map acts on the pair (dz, dq): an entry is a complex 2 x 2 matrix M, a complex
2-vector B and a radius that bounds the pair.

- dcmax / bla_table: the constant (the ship's) and the levels k = 1 .. K of the table, as the device builds them;
- perturb_bla: the per-sample step with BLA and the pair rebase; returns the (iter, r2, lastZ) planes and the three step counts;
- samples_bla / restate_bla: every sub-sample of a frame, the counts summed (fr_ctx_last_deep_phoenix_steps), and the planes.

deep_phoenix_ref.py supplies the orbit, the sample offsets, the plain step's restatement and the colour stage; deep_bla_ref.py
the level arithmetic all tables share.
"""
from __future__ import annotations

import numpy as np

import deep_phoenix_ref as D
import deep_ship_ref as S
from deep_bla_ref import EPS, _ctz, _flog2, levels
from deep_ship_bla_ref import dcmax                                # the ship's, operation for operation

F32 = np.float32
ELEMS = ("m11", "m12", "m21", "m22", "b1", "b2")                   # the order of an entry's six complex numbers
ENTRY_DOUBLES = 12


def _cmul(a, b):
    """a * b = (a.x b.x - a.y b.y, a.x b.y + a.y b.x)"""
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def _cadd(a, b):
    return a[0] + b[0], a[1] + b[1]


def _n2(c):
    """|c|^2 = c.x c.x + c.y c.y"""
    return c[0] * c[0] + c[1] * c[1]


def single_steps(orbit: np.ndarray, p: float, r: float, eps: float = EPS) -> dict:
    """The single steps m = 1 .. N - 1 (never stored on the device): a = ((Z.x + Z.x) + p, Z.y + Z.y), M = (a, (r, 0), (1, 0), 0),
    B = ((1, 0), 0), rad = (0.5 eps) |a|"""
    N = len(orbit) - 1
    X, Y = orbit[1:N, 0].copy(), orbit[1:N, 1].copy()
    p, r = np.float64(F32(p)), np.float64(F32(r))
    ax, ay = (X + X) + p, Y + Y
    one, zero = np.ones_like(X), np.zeros_like(X)
    return dict(r=(np.float64(0.5) * np.float64(eps)) * np.sqrt(ax * ax + ay * ay), m11=(ax, ay), m12=(zero + r, zero),
                m21=(one, zero), m22=(zero, zero), b1=(one, zero), b2=(zero, zero))


def bla_table(orbit: np.ndarray, dcm: float, p: float, r: float, eps: float = EPS):
    """Levels 1 .. K: a list of dicts (index k - 1) with the array r and the six complex elements (pairs of arrays) over the
    entries j of the level, entry j covering the 2^k steps from m = 1 + j * 2^k"""
    N = len(orbit) - 1
    K = levels(N)
    if K == 0:
        return []
    with np.errstate(all="ignore"):
        prev = single_steps(orbit, p, r, eps)
        dm = np.float64(dcm)
        out = []
        for k in range(1, K + 1):
            cnt = (N - 1) >> k
            half = lambda v, o: v[o:2 * cnt:2] if isinstance(v, np.ndarray) else (v[0][o:2 * cnt:2], v[1][o:2 * cnt:2])
            x = {q: half(v, 0) for q, v in prev.items()}
            y = {q: half(v, 1) for q, v in prev.items()}
            e = {}
            for i in ("1", "2"):
                for j in ("1", "2"):
                    e["m" + i + j] = _cadd(_cmul(y["m" + i + "1"], x["m1" + j]), _cmul(y["m" + i + "2"], x["m2" + j]))
                e["b" + i] = _cadd(_cadd(_cmul(y["m" + i + "1"], x["b1"]), _cmul(y["m" + i + "2"], x["b2"])), y["b" + i])
            nM = np.sqrt((_n2(x["m11"]) + _n2(x["m12"])) + (_n2(x["m21"]) + _n2(x["m22"])))
            nB = np.sqrt(_n2(x["b1"]) + _n2(x["b2"]))
            t = (y["r"] - nB * dm) / nM
            rad = np.where(t > 0.0, t, 0.0)
            rad = np.where(rad < x["r"], rad, x["r"])
            fin = np.ones(cnt, bool)
            for q in ELEMS:
                fin &= np.isfinite(e[q][0]) & np.isfinite(e[q][1])
            e["r"] = np.where(fin, rad, 0.0)
            prev = e
            out.append(e)
    return out


def table_arrays(table):
    """The table as fr_deep_phoenix_bla_table reads it back: r of every entry, and (n, 12) doubles M11, M12, M21, M22, B1, B2"""
    r = np.concatenate([T["r"] for T in table])
    mb = np.concatenate([np.stack([T[q][c] for q in ELEMS for c in (0, 1)], axis=1) for T in table])
    return r, mb


def perturb_bla(orbit: np.ndarray, dcx: np.ndarray, dcy: np.ndarray, max_iter: int, p: float, r: float, table):
    """The per-sample step of the header with BLA.  Returns (iter, r2, lastZ x, lastZ y, counts): as deep_phoenix_ref.perturb,
    counts = [plain steps, BLA steps, updates skipped] over the samples."""
    ox, oy = np.ascontiguousarray(orbit[:, 0]), np.ascontiguousarray(orbit[:, 1])
    N = len(orbit) - 1
    K = len(table)
    shape = dcx.shape
    cx, cy = dcx.ravel().astype(np.float64), dcy.ravel().astype(np.float64)
    n = cx.size
    p, r = np.float64(F32(p)), np.float64(F32(r))
    rr = r * r
    four = np.float64(4.0)
    it = np.full(n, max_iter, np.int32)
    r2out = np.zeros(n, np.float64)
    ezx = np.zeros(n, np.float64); ezy = np.zeros(n, np.float64)
    idx = np.arange(n)
    dzx = np.zeros(n); dzy = np.zeros(n); dqx = np.zeros(n); dqy = np.zeros(n)
    m = np.zeros(n, np.int64)
    u = np.zeros(n, np.int64)
    counts = [0, 0, 0]
    while idx.size:
        Zx, Zy = ox[m], oy[m]
        n2 = (dzx * dzx + dzy * dzy) + (dqx * dqx + dqy * dqy)
        k = np.zeros(idx.size, np.int64)
        cand = np.nonzero(m >= 1)[0] if K else np.zeros(0, np.int64)
        if cand.size:
            mc = m[cand]
            kk = np.minimum(_ctz(mc - 1, K), K)
            kk = np.minimum(kk, _flog2(N - mc))
            kk = np.minimum(kk, _flog2(max_iter - u[cand]))
            for lvl in range(K, 0, -1):                               # top down: the largest valid k (radii are monotone in k)
                sel = np.nonzero(kk == lvl)[0]
                if sel.size == 0:
                    continue
                rad = table[lvl - 1]["r"][(mc[sel] - 1) >> lvl]
                bad = ~(n2[cand[sel]] < rad * rad)
                kk[sel[bad]] -= 1
            k[cand] = np.maximum(kk, 0)
        bl = k > 0
        tx = ((Zx + Zx) + dzx) + p                                   # the plain step, as deep_phoenix_ref.perturb
        ty = (Zy + Zy) + dzy
        nx = ((tx * dzx - ty * dzy) + r * dqx) + cx
        ny = ((tx * dzy + ty * dzx) + r * dqy) + cy
        nqx, nqy = dzx.copy(), dzy.copy()                            # dq'
        if bl.any():
            b = np.nonzero(bl)[0]
            kb = k[b]
            j = (m[b] - 1) >> kb
            E = {q: (np.empty(b.size), np.empty(b.size)) for q in ELEMS}
            for lvl in np.unique(kb):
                s = kb == lvl
                T = table[lvl - 1]
                for q in ELEMS:
                    E[q][0][s] = T[q][0][j[s]]
                    E[q][1][s] = T[q][1][j[s]]
            dz, dq, dc = (dzx[b], dzy[b]), (dqx[b], dqy[b]), (cx[b], cy[b])
            nz = _cadd(_cadd(_cmul(E["m11"], dz), _cmul(E["m12"], dq)), _cmul(E["b1"], dc))
            nq = _cadd(_cadd(_cmul(E["m21"], dz), _cmul(E["m22"], dq)), _cmul(E["b2"], dc))
            nx[b], ny[b] = nz
            nqx[b], nqy[b] = nq
        step = np.where(bl, np.left_shift(1, k), 1)
        counts[0] += int((~bl).sum())
        counts[1] += int(bl.sum())
        counts[2] += int(step[bl].sum())
        m = m + step
        u = u + step
        zx, zy = ox[m] + nx, oy[m] + ny
        qx, qy = ox[m - 1] + nqx, oy[m - 1] + nqy
        r2 = zx * zx + zy * zy
        esc = r2 > four
        small = (r2 + rr * (qx * qx + qy * qy)) < ((nx * nx + ny * ny) + rr * (nqx * nqx + nqy * nqy))
        reb = ~esc & (small | (m == N))
        dzx = np.where(reb, zx, nx); dzy = np.where(reb, zy, ny)
        dqx = np.where(reb, qx, nqx); dqy = np.where(reb, qy, nqy)
        m = np.where(reb, 0, m)
        e = idx[esc]
        it[e] = (u[esc] - 1).astype(np.int32)
        r2out[e] = r2[esc]
        ezx[e] = zx[esc]; ezy[e] = zy[esc]
        done = ~esc & (u >= max_iter)                                 # lastZ of a sample that never escaped: Z_m + dz
        e = idx[done]
        ezx[e] = ox[m[done]] + dzx[done]; ezy[e] = oy[m[done]] + dzy[done]
        keep = ~esc & ~done
        if not keep.all():
            idx, dzx, dzy, dqx, dqy = idx[keep], dzx[keep], dzy[keep], dqx[keep], dqy[keep]
            m, u, cx, cy = m[keep], u[keep], cx[keep], cy[keep]
    return it.reshape(shape), r2out.reshape(shape), ezx.reshape(shape), ezy.reshape(shape), counts


def view_table(view: dict, W: int, H: int, orbit=None, eps: float = EPS):
    """The table of a view's frame; dcmax is that of the whole W x H frame"""
    if orbit is None:
        orbit = D.view_orbit(view)
    return bla_table(orbit, dcmax(W, H, view["zoom"]), view["p"], view["r"], eps)


def samples_bla(view: dict, W: int, H: int, aa: int = 1, rows=None, orbit=None, eps: float = EPS):
    """Every sub-sample of the frame (or of its rows), sx outer: a list over s of (iter, r2, lastZ x, lastZ y) planes, as
    deep_phoenix_ref.samples, and the three counts summed.  dcmax is that of the whole W x H frame, whatever the rows."""
    if orbit is None:
        orbit = D.view_orbit(view)
    table = view_table(view, W, H, orbit, eps)
    n_aa = max(int(aa), 1)
    out, total = [], [0, 0, 0]
    for s in range(n_aa * n_aa):
        dcx, dcy = S.sample_dc(W, H, view["zoom"], n_aa, s, rows)
        it, r2, ezx, ezy, c = perturb_bla(orbit, dcx, dcy, view["max_iter"], view["p"], view["r"], table)
        out.append((it, r2, ezx, ezy))
        total = [a + b for a, b in zip(total, c)]
    return out, total


def restate_bla(view: dict, W: int, H: int, aa: int = 1, density: float = 0.0, post: bool = False, rows=None, orbit=None):
    """A frame (or its rows): (iter, nu, rgb, counts) -- iter / nu of sample (0,0), rgb of all of them, the colour stage being
    deep_phoenix_ref's"""
    smp, counts = samples_bla(view, W, H, aa, rows, orbit)
    it, _, ezx, ezy = smp[0]
    return it, D.smooth(it, ezx, ezy, view["max_iter"]), D.colour(smp, view["max_iter"], density, post), counts
