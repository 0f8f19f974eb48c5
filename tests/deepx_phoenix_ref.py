"""Deep Phoenix views with extended-exponent deltas (fr_render_deepx_phoenix): ground truth with nothing but Python integers
and numpy, next to deep_phoenix_ref (the recurrence, the pair rebase rule, the colour stage) and deepx_ref (the extended
arithmetic).  TEST INFRASTRUCTURE ONLY.

- fixed_orbit / reference_orbit_x: the fixed-point orbit of z' = z^2 + c + r z_prev + p z in the extended storage;
- perturb_x: the kernel's two-mode per-sample step, op for op the header's EXTENDED and PLAIN steps;
- restate_x: iter, smooth count and colour planes of a frame;
- exact_iter_x / exact_frame_x: the direct iteration of one sample in fixed point at F + 64 fraction bits, dc exactly;
- exact_golden: the exact frames of the new views at 24x18, recorded in tests/golden/deepx_phoenix_exact.npz by
  tests/golden/make_deepx_phoenix_golden.py (each takes 10 to 40 s; the host tests recompute a sample of their pixels).
"""
from __future__ import annotations

import os
from decimal import ROUND_HALF_EVEN, Decimal, localcontext
from fractions import Fraction

import numpy as np

import deep_phoenix_ref as P
import deep_ref as R
import deep_ship_ref as S
import deepx_ref as X
import deepx_ship_ref as SX
from deepx_ref import X_THR, X_ZERO, _THR, _ld, _norm

F32 = np.float32
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# PX400A / PX400B: deep_phoenix_ref's PA / PB followed down to 1e-400 by the same search (10x zooms onto the boundary with exact
# integer iteration); max_iter 300 above the centre's escape index.
PX400A = dict(
    cx="-1.2360060287158406444212431573932696136124674314980456879500438835572038736806089252982094115419307306804402528776484816655816676667985139232534268046412892520691139613721142688681003934192137607996130693823372712313378261760870934238502507640592173900669089373303358348428003622619442558278070084128098110492260894584741660024495962741726226957959073975050742963990999419350173848403329675733864825157589285714286",
    cy="0.3165380442307620550110322882934310805622698622468650000451551526262733746249906090393244239487019669028569871855688234760742825657938883547614443297767842857142857330002714279811442867000033662133931718554400003725767858571428571714284318856713985728572831065500004281428542553104256997237203348500410625118424145898571011449299998985740981458928430243065931142857143160290178114426971428824582859971428571428571",
    zoom="1e-400", max_iter=3525, p=0.0, r=-0.5)
PX400B = dict(
    cx="-0.9351332846815240128006232081244435623888608659049737155689347616703275138358626281068795002169159545250000810247884654292655191518442544325720746747639226604267074239001439613469138609965170621570779337917467927757830992734441618693421459764640595315198044197189732140355092424398140132700358839077582535438947059085713479744175295668046492641957844061125313179560718723588153478591098948832733045452008928571429",
    cy="0.5110737514852719620399989262479350186710450720721156412590302160910019374276376851437496251636353201499981714285571428412817410308035739049028244742818573142385713857003472785433286997447114004143171414300287130014311285739982871571414714272857144560004285999557128573243142966800042857125714289001425755805531046356675383045988745631692314394628156854248946041428457104910288814288555745826767867157142857142857",
    zoom="1e-400", max_iter=5355, p=0.25, r=-0.375)


def _round_decimals(s: str, places: int) -> str:
    with localcontext() as ctx:
        ctx.prec = len(s) + 8
        return str(Decimal(s).quantize(Decimal(1).scaleb(-places), rounding=ROUND_HALF_EVEN))


# PX310: PX400A's strings rounded to 322 decimals
PX310 = dict(cx=_round_decimals(PX400A["cx"], 322), cy=_round_decimals(PX400A["cy"], 322), zoom="1e-310", max_iter=2877, p=0.0,
             r=-0.5)
# TIP1000: the Mandelbrot tip (p = r = 0), Y exactly zero, exponents down to 2^-3322.  The centre is -2 + 6.72e-1001: the tip
# itself lies 0.1 pixel spacings left of the first column of a 24x18 frame.  Centred on -2, half the frame has |c| > 2 and
# escapes at index 0 by a margin of 1e-1000, which no 53-bit z = Z_1 + dz can show (|z|^2 rounds to 4); moved right, every pixel has
# Re c > -2, row H/2 is the antenna itself (interior), and the exact iteration shows 8 escape indices, 1660 .. 1667.
TIP1000 = dict(cx="-1." + "9" * 1000 + "328", cy="0", zoom="1e-1000", max_iter=2400, p=0.0, r=0.0)
# PXRET: PX400A's centre at a zoom at which most lanes of a 24x18 frame turn plain and fall back to the extended mode at least
# once (367 of 432 in the restatement): the plain-to-extended block of the Phoenix loop with r != 0, dq normalised with dz.
# The strings are rounded to 342 decimals as PX310's are to 322: PX400A's centre lies within 1e-400 of the boundary, the
# sample with dc = 0 is the centre itself, and the orbit (F = 1280 bits) and the exact iteration (F + 64) round a longer
# string to two numbers on either side of that boundary (escape at 2825 against none: measured).
PXRET = dict(PX400A, cx=_round_decimals(PX400A["cx"], 342), cy=_round_decimals(PX400A["cy"], 342), zoom="7e-330")
NEW_VIEWS = {"PX310": PX310, "PX400A": PX400A, "PX400B": PX400B, "TIP1000": TIP1000, "PXRET": PXRET}


def as_x_view(v: dict) -> dict:
    """a deep_phoenix_ref view (zoom a double) as an extended one (zoom its shortest decimal string)"""
    return dict(v, zoom=repr(float(v["zoom"])))


# the fp64 views fr_render_deep_phoenix renders, passed as extended views
OLD_VIEWS = {k: as_x_view(P.VIEWS[k]) for k in ("PA30", "PB30", "PA", "PB", "shallowA", "miniR")}


def frac_bits_of(view: dict) -> int:
    return view.get("frac_bits") or X.frac_bits_x(view["zoom"])


def fixed_orbit(cx: str, cy: str, F: int, max_iter: int, p: float, r: float):
    """Z_0 .. Z_N as Python integers (value 2^F): deep_phoenix_ref.reference_orbit's recurrence"""
    Cr, Ci = R.parse_fixed(cx, F), R.parse_fixed(cy, F)
    Pp, Rr = P._fixed_floor(p, F), P._fixed_floor(r, F)
    T = 4 << (2 * F)
    zr = zi = qr = qi = 0
    out = [(0, 0)]
    for _ in range(max_iter):
        sr, si = zr * zr, zi * zi
        if sr + si > T:
            break
        nr = (sr >> F) - (si >> F) + Cr + ((Rr * qr) >> F) + ((Pp * zr) >> F)
        ni = ((2 * zr * zi) >> F) + Ci + ((Rr * qi) >> F) + ((Pp * zi) >> F)
        qr, qi, zr, zi = zr, zi, nr, ni
        out.append((zr, zi))
    return out


def reference_orbit_x(cx: str, cy: str, F: int, max_iter: int, p: float, r: float):
    pts = [X.store_point(zr, zi, F) for zr, zi in fixed_orbit(cx, cy, F, max_iter, p, r)]
    return np.array([(q[0], q[1]) for q in pts], np.float64), np.array([q[2] for q in pts], np.int32)


def orbit_of(view: dict):
    return reference_orbit_x(view["cx"], view["cy"], frac_bits_of(view), view["max_iter"], view["p"], view["r"])


def perturb_x(mant, exp2, dc, max_iter: int, p: float, r: float, stats=None):
    """The two-mode step of the header on flat sample arrays.  Returns (iter, lastZ x, lastZ y).  stats: ext_steps, plain_steps,
    to_plain, to_ext, rebases."""
    omx, omy = np.ascontiguousarray(mant[:, 0]), np.ascontiguousarray(mant[:, 1])
    oe = exp2.astype(np.int64)
    plain = X.decode(mant, exp2)
    opx, opy = np.ascontiguousarray(plain[:, 0]), np.ascontiguousarray(plain[:, 1])
    N = len(oe) - 1
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
    n_ext = n_plain = to_plain = to_ext = n_reb = 0
    with np.errstate(all="ignore"):
        for i in range(max_iter):
            if idx.size == 0:
                break
            esc = np.zeros(idx.size, bool)
            lzx = np.zeros(idx.size); lzy = np.zeros(idx.size)
            E = np.nonzero(ext)[0]
            Q = np.nonzero(~ext)[0]
            if E.size:
                n_ext += E.size
                mm = m[E]
                Zx, Zy, eZ = omx[mm], omy[mm], oe[mm]
                a, b, e = dx[E], dy[E], ed[E]
                c, d, f = qx_[E], qy_[E], eq[E]
                eu = np.maximum(eZ + 1, e)
                ux = _ld(Zx, eZ + 1 - eu) + _ld(a, e - eu)
                uy = _ld(Zy, eZ + 1 - eu) + _ld(b, e - eu)
                et = np.maximum(eu, pe)
                tx = _ld(ux, eu - et) + _ld(np.full(E.size, p), pe - et)
                ty = _ld(uy, eu - et)
                px = tx * a - ty * b
                py = tx * b + ty * a
                ep = et + e
                er = np.full(E.size, X_ZERO, np.int64) if r == 0.0 else f
                e1 = np.maximum(ep, er)
                sx = _ld(px, ep - e1) + _ld(r * c, er - e1)
                sy = _ld(py, ep - e1) + _ld(r * d, er - e1)
                en = np.maximum(e1, ec[E])
                nx = _ld(sx, e1 - en) + _ld(cx[E], ec[E] - en)
                ny = _ld(sy, e1 - en) + _ld(cy[E], ec[E] - en)
                mm = mm + 1
                Wx, Wy, eW = omx[mm], omy[mm], oe[mm]
                ez = np.maximum(eW, en)
                zx = _ld(Wx, eW - ez) + _ld(nx, en - ez)
                zy = _ld(Wy, eW - ez) + _ld(ny, en - ez)
                eqq = np.maximum(eZ, e)
                qx = _ld(Zx, eZ - eqq) + _ld(a, e - eqq)
                qy = _ld(Zy, eZ - eqq) + _ld(b, e - eqq)
                r2 = zx * zx + zy * zy
                es = _ld(r2, 2 * ez) > four
                lhs = r2 + _ld(rr * (qx * qx + qy * qy), 2 * (eqq - ez))
                rhs = _ld(nx * nx + ny * ny, 2 * (en - ez)) + _ld(rr * (a * a + b * b), 2 * (e - ez))
                reb = ~es & ((lhs < rhs) | (mm == N))
                n_reb += int(reb.sum())
                ax, ay, ea = _norm(np.where(reb, zx, nx), np.where(reb, zy, ny), np.where(reb, ez, en))
                nqx = np.where(reb, qx, a); nqy = np.where(reb, qy, b)
                nqe = np.where(reb, np.where((qx == 0.0) & (qy == 0.0), X_ZERO, eqq), e)
                stay = ea <= X_THR
                to_plain += int((~stay & ~es).sum())
                dx[E] = np.where(stay, ax, _ld(ax, np.where(stay, 0, ea)))
                dy[E] = np.where(stay, ay, _ld(ay, np.where(stay, 0, ea)))
                ed[E] = ea
                qx_[E] = np.where(stay, nqx, _ld(nqx, np.where(stay, 0, nqe)))
                qy_[E] = np.where(stay, nqy, _ld(nqy, np.where(stay, 0, nqe)))
                eq[E] = nqe
                ext[E] = stay
                m[E] = np.where(reb, 0, mm)
                esc[E] = es
                lzx[E] = _ld(zx, ez); lzy[E] = _ld(zy, ez)
            if Q.size:
                n_plain += Q.size
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
                n_reb += int(reb.sum())
                ax = np.where(reb, zx, nx); ay = np.where(reb, zy, ny)
                nqx = np.where(reb, qx, a); nqy = np.where(reb, qy, b)
                small = np.maximum(np.abs(ax), np.abs(ay)) < _THR
                to_ext += int((small & ~es).sum())
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
            if esc.any():
                e_ = idx[esc]
                it[e_] = i
                ezx[e_] = lzx[esc]; ezy[e_] = lzy[esc]
                k = ~esc
                idx, dx, dy, ed, qx_, qy_, eq, ext, m = idx[k], dx[k], dy[k], ed[k], qx_[k], qy_[k], eq[k], ext[k], m[k]
                cx, cy, ec, cpx, cpy = cx[k], cy[k], ec[k], cpx[k], cpy[k]
        # lastZ of a sample that never escaped: Z_m (+) dz of its final state, as a double
        if idx.size:
            eZ = oe[m]
            ez = np.maximum(eZ, ed)
            lx = _ld(_ld(omx[m], eZ - ez) + _ld(dx, ed - ez), ez)
            ly = _ld(_ld(omy[m], eZ - ez) + _ld(dy, ed - ez), ez)
            ezx[idx] = np.where(ext, lx, opx[m] + dx)
            ezy[idx] = np.where(ext, ly, opy[m] + dy)
    if stats is not None:
        for key, v in (("ext_steps", n_ext), ("plain_steps", n_plain), ("to_plain", to_plain), ("to_ext", to_ext),
                       ("rebases", n_reb)):
            stats[key] = stats.get(key, 0) + v
    return it, ezx, ezy


def samples_x(view: dict, W: int, H: int, aa: int = 1, rows=None, orbit=None, stats=None):
    """Every sub-sample of the frame (or of its rows), sx outer: a list over s of (iter, r2, lastZ x, lastZ y) planes in
    deep_phoenix_ref.samples' layout (r2 = |lastZ|^2, 0 for interior)"""
    mant, exp2 = orbit if orbit is not None else orbit_of(view)
    zm, ze = X.zoom_pair(view["zoom"])
    nrows = H if rows is None else len(rows)
    n_aa = max(int(aa), 1)
    ns = n_aa * n_aa
    dcs = [SX.sample_dc_ship_x(W, H, zm, ze, n_aa, s, rows) for s in range(ns)]
    dc = tuple(np.concatenate([d[k] for d in dcs]) for k in range(5))     # the samples are independent: one pass over all of them
    it, ezx, ezy = perturb_x(mant, exp2, dc, view["max_iter"], view["p"], view["r"], stats)
    r2 = np.where(it < view["max_iter"], ezx * ezx + ezy * ezy, 0.0)
    return [tuple(a.reshape(ns, nrows, W)[s] for a in (it, r2, ezx, ezy)) for s in range(ns)]


def restate_x(view: dict, W: int, H: int, aa: int = 1, density: float = 0.0, post: bool = False, rows=None, orbit=None,
              stats=None):
    """A frame (or its rows): (iter, nu, rgb) -- iter / nu of sample (0,0), rgb of all of them"""
    smp = samples_x(view, W, H, aa, rows, orbit, stats)
    it, _, ezx, ezy = smp[0]
    return it, P.smooth(it, ezx, ezy, view["max_iter"]), P.colour(smp, view["max_iter"], density, post)


def exact_iter_x(view: dict, x: int, y: int, W: int, H: int) -> int:
    """The escape index of sample (x, y), aa 1, by the direct iteration of the recurrence in fixed point at F + 64 fraction
    bits; dc = the map on zm, rounded to double as the kernel forms it, times 2^ze exactly; p and r exactly"""
    zm, ze = X.zoom_pair(view["zoom"])
    G = frac_bits_of(view) + 64
    mx, my = S.sample_dc(W, H, zm, 1, 0, rows=[y])
    s = Fraction(2) ** ze
    cr = round((Fraction(view["cx"]) + Fraction(float(mx[0, x])) * s) * (1 << G))
    ci = round((Fraction(view["cy"]) + Fraction(float(my[0, x])) * s) * (1 << G))
    Pp, Rr = P._fixed_floor(view["p"], G), P._fixed_floor(view["r"], G)
    T = 4 << (2 * G)
    zr = zi = qr = qi = 0
    for i in range(view["max_iter"]):
        nr = ((zr * zr - zi * zi + Rr * qr + Pp * zr) >> G) + cr
        ni = ((2 * zr * zi + Rr * qi + Pp * zi) >> G) + ci
        qr, qi, zr, zi = zr, zi, nr, ni
        if zr * zr + zi * zi > T:
            return i
    return view["max_iter"]


def exact_frame_x(view: dict, W: int, H: int) -> np.ndarray:
    """exact_iter_x of every pixel"""
    return np.array([[exact_iter_x(view, x, y, W, H) for x in range(W)] for y in range(H)], np.int32)


GOLDEN_SIZE = (24, 18)


def exact_golden() -> dict:
    """name -> exact_frame_x(view, 24, 18) of the new views, as recorded"""
    with np.load(os.path.join(_GOLDEN, "deepx_phoenix_exact.npz")) as z:
        return {k: z[k] for k in z.files}
