"""Deep Burning Ship views with bilinear approximation (fr_render_deep_ship with FR_FLAG_DEEP_SHIP_BLA): the table build and
the stepping of the header, restated operation for operation in fp64 numpy, vectorised over samples.

- dcmax / bla_table: the constants and the levels k = 1 .. K of the table, as the device builds them;
- perturb_bla: the per-sample step with BLA and rebasing; returns the (iter, r2) planes and the three step counts;
- restate_bla: every sub-sample of a frame, the counts summed (fr_ctx_last_deep_ship_steps).

deep_ship_ref.py supplies the ship's reference orbit, the sample offsets, the fold, the smooth count and the exact
fixed-point iteration; deep_bla_ref.py the level arithmetic the two tables share.
"""
from __future__ import annotations

import numpy as np

import deep_ship_ref as S
from deep_bla_ref import EPS, _ctz, _flog2, levels

ELEMS = ("a11", "a12", "a21", "a22", "b11", "b12", "b21", "b22")     # the order of an entry's eight doubles


def dcmax(W: int, H: int, zoom: float) -> float:
    """(1.0000001 * zoom) * sqrt(ex*ex + hy*hy) of the whole frame: hx = 0.5 + 0.5 / (W*W), hy = 0.5 + 0.5 / (W*H),
    ex = hx * (W / H) -- the ship shader's sub-sample offsets leave [0, 1) by up to (aa-1)/(2 aa W^2) and (aa-1)/(2 aa W H)"""
    f = np.float64
    a = f(W) / f(H)
    hx = f(0.5) + f(0.5) / (f(W) * f(W))
    hy = f(0.5) + f(0.5) / (f(W) * f(H))
    ex = hx * a
    return float((f(1.0000001) * f(zoom)) * np.sqrt(ex * ex + hy * hy))


def single_steps(orbit: np.ndarray, eps: float = EPS) -> dict:
    """The single steps m = 1 .. N - 1 (never stored on the device): A = [[2X, -2Y], [2|Y| sgn X, 2|X| sgn Y]], B = 1,
    r = eps |Z_m| capped by |X| and |Y| (the fold conditions)"""
    N = len(orbit) - 1
    X, Y = orbit[1:N, 0].copy(), orbit[1:N, 1].copy()
    sx = np.where(X >= 0.0, 1.0, -1.0)
    sy = np.where(Y >= 0.0, 1.0, -1.0)
    aX, aY = np.abs(X), np.abs(Y)
    r = np.float64(eps) * np.sqrt(X * X + Y * Y)
    r = np.where(r < aX, r, aX)
    r = np.where(r < aY, r, aY)
    return dict(r=r, a11=X + X, a12=-(Y + Y), a21=(aY + aY) * sx, a22=(aX + aX) * sy,
                b11=np.ones_like(X), b12=np.zeros_like(X), b21=np.zeros_like(X), b22=np.ones_like(X))


def bla_table(orbit: np.ndarray, dcm: float, eps: float = EPS):
    """Levels 1 .. K: a list of dicts (index k - 1) with arrays r and the eight elements over the entries j of the level,
    entry j covering the 2^k steps from m = 1 + j * 2^k"""
    N = len(orbit) - 1
    K = levels(N)
    if K == 0:
        return []
    with np.errstate(all="ignore"):
        prev = single_steps(orbit, eps)
        dm = np.float64(dcm)
        out = []
        for k in range(1, K + 1):
            cnt = (N - 1) >> k
            x = {q: v[0:2 * cnt:2] for q, v in prev.items()}
            y = {q: v[1:2 * cnt:2] for q, v in prev.items()}
            a11 = y["a11"] * x["a11"] + y["a12"] * x["a21"]
            a12 = y["a11"] * x["a12"] + y["a12"] * x["a22"]
            a21 = y["a21"] * x["a11"] + y["a22"] * x["a21"]
            a22 = y["a21"] * x["a12"] + y["a22"] * x["a22"]
            b11 = (y["a11"] * x["b11"] + y["a12"] * x["b21"]) + y["b11"]
            b12 = (y["a11"] * x["b12"] + y["a12"] * x["b22"]) + y["b12"]
            b21 = (y["a21"] * x["b11"] + y["a22"] * x["b21"]) + y["b21"]
            b22 = (y["a21"] * x["b12"] + y["a22"] * x["b22"]) + y["b22"]
            nB = np.sqrt((x["b11"] * x["b11"] + x["b12"] * x["b12"]) + (x["b21"] * x["b21"] + x["b22"] * x["b22"]))
            nA = np.sqrt(x["a11"] * x["a11"] + x["a21"] * x["a21"])
            t = (y["r"] - nB * dm) / nA
            r = np.where(t > 0.0, t, 0.0)
            r = np.where(r < x["r"], r, x["r"])
            fin = np.ones(cnt, bool)
            for v in (a11, a12, a21, a22, b11, b12, b21, b22):
                fin &= np.isfinite(v)
            r = np.where(fin, r, 0.0)
            prev = dict(r=r, a11=a11, a12=a12, a21=a21, a22=a22, b11=b11, b12=b12, b21=b21, b22=b22)
            out.append(prev)
    return out


def perturb_bla(orbit: np.ndarray, dcx: np.ndarray, dcy: np.ndarray, max_iter: int, table, bailout: float = 4.0):
    """The per-sample step of the header with BLA.  Returns (iter, r2, counts): iter = the escape index (max_iter if
    none), r2 = |z|^2 there, counts = [plain steps, BLA steps, updates skipped] over the samples."""
    ox, oy = np.ascontiguousarray(orbit[:, 0]), np.ascontiguousarray(orbit[:, 1])
    N = len(orbit) - 1
    K = len(table)
    B2 = np.float64(np.float32(bailout)) * np.float64(np.float32(bailout))
    shape = dcx.shape
    cx, cy = dcx.ravel().astype(np.float64), dcy.ravel().astype(np.float64)
    n = cx.size
    it = np.full(n, max_iter, np.int32)
    r2out = np.zeros(n, np.float64)
    idx = np.arange(n)
    dzx = np.zeros(n); dzy = np.zeros(n)
    m = np.zeros(n, np.int64)
    u = np.zeros(n, np.int64)
    counts = [0, 0, 0]
    while idx.size:
        Zx, Zy = ox[m], oy[m]
        dz2 = dzx * dzx + dzy * dzy
        k = np.zeros(idx.size, np.int64)
        if K:
            # r of every level at m is <= eps |Z_m|: only samples below that can take a BLA step
            r0 = np.float64(EPS) * np.sqrt(Zx * Zx + Zy * Zy)
            cand = np.nonzero((m >= 1) & (dz2 < r0 * r0))[0]
            if cand.size:
                mc = m[cand]
                kk = np.minimum(_ctz(mc - 1, K), K)
                kk = np.minimum(kk, _flog2(N - mc))
                kk = np.minimum(kk, _flog2(max_iter - u[cand]))
                for lvl in range(K, 0, -1):                           # top down: the largest valid k
                    sel = np.nonzero(kk == lvl)[0]
                    if sel.size == 0:
                        continue
                    r = table[lvl - 1]["r"][(mc[sel] - 1) >> lvl]
                    bad = ~(dz2[cand[sel]] < r * r)
                    kk[sel[bad]] -= 1
                k[cand] = np.maximum(kk, 0)
        bl = k > 0
        fx, fy = S.fold(Zx, dzx), S.fold(Zy, dzy)                      # the ship's plain step, as deep_ship_ref.perturb
        tx = (np.abs(Zx) + np.abs(Zx)) + fx
        ty = (np.abs(Zy) + np.abs(Zy)) + fy
        nx = (tx * fx - ty * fy) + cx
        ny = (tx * fy + ty * fx) + cy
        if bl.any():
            b = np.nonzero(bl)[0]
            kb = k[b]
            j = (m[b] - 1) >> kb
            E = {q: np.empty(b.size) for q in ELEMS}
            for lvl in np.unique(kb):
                s = kb == lvl
                T = table[lvl - 1]
                for q in ELEMS:
                    E[q][s] = T[q][j[s]]
            ex, ey, gx, gy = dzx[b], dzy[b], cx[b], cy[b]
            nx[b] = (E["a11"] * ex + E["a12"] * ey) + (E["b11"] * gx + E["b12"] * gy)
            ny[b] = (E["a21"] * ex + E["a22"] * ey) + (E["b21"] * gx + E["b22"] * gy)
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
        keep = ~esc & (u < max_iter)
        if not keep.all():
            idx, dzx, dzy, m, u, cx, cy = idx[keep], dzx[keep], dzy[keep], m[keep], u[keep], cx[keep], cy[keep]
    return it.reshape(shape), r2out.reshape(shape), counts


def restate_bla(view: dict, W: int, H: int, aa: int = 1, bailout: float = 4.0, rows=None, orbit=None, eps: float = EPS):
    """Every sub-sample of the frame (or of its rows): a list over s of (iter, r2) planes, and the three counts summed.
    dcmax is that of the whole W x H frame, whatever the rows."""
    if orbit is None:
        orbit = S.reference_orbit(view["cx"], view["cy"], view["zoom"], view["max_iter"], bailout)
    table = bla_table(orbit, dcmax(W, H, view["zoom"]), eps)
    out, total = [], [0, 0, 0]
    for s in range(aa * aa):
        dcx, dcy = S.sample_dc(W, H, view["zoom"], aa, s, rows)
        it, r2, c = perturb_bla(orbit, dcx, dcy, view["max_iter"], table, bailout)
        out.append((it, r2))
        total = [a + b for a, b in zip(total, c)]
    return out, total
