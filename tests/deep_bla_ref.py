"""Deep Mandelbrot views with bilinear approximation (fr_render_deep with FR_FLAG_DEEP_BLA): the table build and the
stepping of the header, restated operation for operation in fp64 numpy, vectorised over samples.

- dcmax / bla_table: the constants and the levels k = 1 .. K of the table, as the device builds them;
- perturb_bla: the per-sample step with BLA and rebasing; returns the (iter, r2) planes and the three step counts;
- restate_bla: every sub-sample of a frame, the counts summed (fr_ctx_last_deep_steps);
- VIEW_C: a deep view next to a minibrot (how it was found: below).

deep_ref.py supplies the reference orbit, the sample offsets, the smooth count and the exact fixed-point iteration.
"""
from __future__ import annotations

import numpy as np

import deep_ref as R

EPS = 2.0 ** -53

# View C: next to a minibrot of period 201 at depth 1e-50.  Its nucleus c_201 (z_201(c) = 0) was found by Newton's method
# at 200 digits (mpmath, on the host) on z_201(c) with dz/dc, started from the Misiurewicz point M_{3,1} of views A and B
# plus (1e-40, 1e-40); the nuclei of periods 200 .. 215 found that way lie 7e-26 .. 1e-27 from M_{3,1}, and the size
# estimate of this one's minibrot, 1 / |b l^2| (l = prod 2 z_i, b = sum 1 / prod, i < 201), is 4.4e-51.  The view is
# offset from the nucleus by (0.071, 0.043) view heights, as A and B are from M_{3,1}; its strings are the offset centre
# to 72 significant digits.  The reference orbit does not escape (N = max_iter) and returns near 0 every 201 steps, so
# samples rebase about once per period and BLA can skip most of each.  At 256 x 192, aa 1: 77 % of the samples escape
# and 23 % reach max_iter.
VIEW_C = dict(cx="-0.101096363845622161025785392220571915821120946606593684650467068104296469",
              cy="0.956286510809141500771096045317869046652454388042611743894282235744677940",
              zoom=1e-50, max_iter=8000)


def _abs(x, y):
    """|w| = sqrt(w.x*w.x + w.y*w.y), each operation one rounding (numpy's sqrt is correctly rounded)"""
    return np.sqrt(x * x + y * y)


def dcmax(W: int, H: int, zoom: float) -> float:
    """1.0000001 * (0.5 * zoom) * sqrt((W/H)*(W/H) + 1) of the whole frame, left to right"""
    a = np.float64(W) / np.float64(H)
    return float((np.float64(1.0000001) * (np.float64(0.5) * np.float64(zoom))) * np.sqrt(a * a + np.float64(1.0)))


def levels(N: int) -> int:
    """K = floor(log2(N - 1)); 0 (no table) for N <= 2"""
    return (N - 1).bit_length() - 1 if N > 1 else 0


def bla_table(orbit: np.ndarray, dcm: float, eps: float = EPS):
    """Levels 1 .. K: a list of dicts (index k - 1) with arrays r, ax, ay, bx, by over the entries j of the level,
    entry j covering the 2^k steps from m = 1 + j * 2^k"""
    N = len(orbit) - 1
    K = levels(N)
    if K == 0:
        return []
    with np.errstate(all="ignore"):
        zx, zy = orbit[1:N, 0].copy(), orbit[1:N, 1].copy()          # the single steps m = 1 .. N - 1
        prev = dict(r=np.float64(eps) * _abs(zx, zy), ax=zx + zx, ay=zy + zy, bx=np.ones_like(zx), by=np.zeros_like(zx))
        dm = np.float64(dcm)
        out = []
        for k in range(1, K + 1):
            cnt = (N - 1) >> k
            x = {key: v[0:2 * cnt:2] for key, v in prev.items()}
            y = {key: v[1:2 * cnt:2] for key, v in prev.items()}
            ax = y["ax"] * x["ax"] - y["ay"] * x["ay"]
            ay = y["ax"] * x["ay"] + y["ay"] * x["ax"]
            bx = (y["ax"] * x["bx"] - y["ay"] * x["by"]) + y["bx"]
            by = (y["ax"] * x["by"] + y["ay"] * x["bx"]) + y["by"]
            t = (y["r"] - _abs(x["bx"], x["by"]) * dm) / _abs(x["ax"], x["ay"])
            r = np.where(t > 0.0, t, 0.0)
            r = np.where(r < x["r"], r, x["r"])
            fin = np.isfinite(ax) & np.isfinite(ay) & np.isfinite(bx) & np.isfinite(by)
            r = np.where(fin, r, 0.0)
            prev = dict(r=r, ax=ax, ay=ay, bx=bx, by=by)
            out.append(prev)
    return out


def _ctz(x: np.ndarray, K: int) -> np.ndarray:
    """count of trailing zero bits, K for x == 0"""
    low = x & -x
    out = np.full(x.shape, K, np.int64)
    nz = low > 0
    out[nz] = np.log2(low[nz].astype(np.float64)).astype(np.int64)
    return out


def _flog2(x: np.ndarray) -> np.ndarray:
    """floor(log2(x)) of integers x >= 1"""
    return np.floor(np.log2(x.astype(np.float64))).astype(np.int64)


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
            # r of every level at m is <= r of the single step at m: only samples below that can take a BLA step
            r0 = np.float64(EPS) * _abs(Zx, Zy)             # (the tables of eps <= EPS included)
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
                s = kb == lvl
                T = table[lvl - 1]
                ax[s], ay[s], bx[s], by[s] = T["ax"][j[s]], T["ay"][j[s]], T["bx"][j[s]], T["by"][j[s]]
            ex, ey, gx, gy = dzx[b], dzy[b], cx[b], cy[b]
            nx[b] = (ax * ex - ay * ey) + (bx * gx - by * gy)
            ny[b] = (ax * ey + ay * ex) + (bx * gy + by * gx)
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
        orbit = R.reference_orbit(view["cx"], view["cy"], view["zoom"], view["max_iter"], bailout)
    table = bla_table(orbit, dcmax(W, H, view["zoom"]), eps)
    out, total = [], [0, 0, 0]
    for s in range(aa * aa):
        dcx, dcy = R.sample_dc(W, H, view["zoom"], aa, s, rows)
        it, r2, c = perturb_bla(orbit, dcx, dcy, view["max_iter"], table, bailout)
        out.append((it, r2))
        total = [a + b for a, b in zip(total, c)]
    return out, total
