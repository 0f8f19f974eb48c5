"""Deep Phoenix views (fr_render_deep_phoenix): ground truth with nothing but Python integers and numpy, next to deep_ref and
deep_ship_ref.  TEST INFRASTRUCTURE ONLY.

- reference_orbit: the header's fixed-point orbit of z' = z^2 + c + r z_prev + p z, in Python ints;
- perturb: the kernel's per-sample step with its pair rebase, vectorised over samples in fp64, op for op the header's;
- restate: iter, smooth count and colour planes of a frame (the colour stage is phoenix_ref's, the fp64 Phoenix path's);
- exact_iter: the direct iteration of one sample in fixed point at F + 64 fraction bits (no perturbation at all).

dc is deep_ship_ref.sample_dc: the Phoenix shader's viewport map less the centre, sx outer.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import deep_ref as R
import deep_ship_ref as S
import phoenix_ref as PH

F32 = np.float32

# PA / PB: found by repeated 10x zooms onto the latest-escaping pixel, with exact integer iteration; both centres lie next to an
# interior component, so a frame mixes interior pixels with many escape bands.  PA30 / PB30: the same strings cut for 1e-30.
PA_PR = (0.0, -0.5)
PB_PR = (0.25, -0.375)
PA = dict(cx="-1.2360060287158406444212431573932696136124674314980456879500438835572038736806089252982094115419307306750000000000",
          cy="0.3165380442307620550110322882934310805622698622468650000451551526262733746249906090393244239487019669000000000000",
          zoom=1e-100, max_iter=840, p=PA_PR[0], r=PA_PR[1])
PA30 = dict(cx="-1.2360060287158406444212431573933125", cy="0.3165380442307620550110322882934375", zoom=1e-30, max_iter=320,
            p=PA_PR[0], r=PA_PR[1])
PB = dict(cx="-0.9351332846815240128006232081244435623888608659049737155689347616703275138358626281068795002169159545250000000000",
          cy="0.5110737514852719620399989262479350186710450720721156412590302160910019374276376851437496251636353201500000000000",
          zoom=1e-100, max_iter=1400, p=PB_PR[0], r=PB_PR[1])
PB30 = dict(cx="-0.9351332846815240128006232081244375", cy="0.5110737514852719620399989262479375", zoom=1e-30, max_iter=470,
            p=PB_PR[0], r=PB_PR[1])
SHALLOW_A = dict(cx="-0.5", cy="0", zoom=3.0, max_iter=256, p=PA_PR[0], r=PA_PR[1])
SHALLOW_B = dict(cx="-0.5", cy="0", zoom=3.0, max_iter=256, p=PB_PR[0], r=PB_PR[1])
# r -> 0: a Mandelbrot-like period-3 minibrot, where the rule must behave as Mandelbrot's
MINI_0 = dict(cx="-1.7548776662466927", cy="0", zoom=0.08, max_iter=400, p=0.0, r=0.0)
MINI_R = dict(cx="-1.7548776662466927", cy="0", zoom=0.08, max_iter=400, p=0.0, r=-(2.0 ** -10))
DEEP_VIEWS = {"PA30": PA30, "PB30": PB30, "PA": PA, "PB": PB}
VIEWS = {"shallowA": SHALLOW_A, "shallowB": SHALLOW_B, "mini0": MINI_0, "miniR": MINI_R, **DEEP_VIEWS}
# N of the reference orbit, as the issue that introduced the path records them
ORBIT_N = {"PA30": 244, "PB30": 391, "PA": 758, "PB": 1330}


def _fixed_floor(v: float, F: int) -> int:
    """floor(v 2^F) of the exact value of the float v"""
    return math.floor(Fraction(float(F32(v))) * (1 << F))


def reference_orbit(cx: str, cy: str, zoom: float, max_iter: int, p: float, r: float, F: int = 0) -> np.ndarray:
    """Z_0 .. Z_N as an (N + 1, 2) float64 array; >> is Python's arithmetic shift: floor of the signed product"""
    F = F or R.frac_bits(zoom)
    Cr, Ci = R.parse_fixed(cx, F), R.parse_fixed(cy, F)
    P, Rr = _fixed_floor(p, F), _fixed_floor(r, F)
    T = 4 << (2 * F)
    zr = zi = qr = qi = 0
    out = [(0.0, 0.0)]
    for _ in range(max_iter):
        sr, si = zr * zr, zi * zi
        if sr + si > T:
            break
        nr = (sr >> F) - (si >> F) + Cr + ((Rr * qr) >> F) + ((P * zr) >> F)
        ni = ((2 * zr * zi) >> F) + Ci + ((Rr * qi) >> F) + ((P * zi) >> F)
        qr, qi, zr, zi = zr, zi, nr, ni
        out.append((float(Fraction(zr, 1 << F)), float(Fraction(zi, 1 << F))))
    return np.array(out, dtype=np.float64)


def perturb(orbit: np.ndarray, dcx: np.ndarray, dcy: np.ndarray, max_iter: int, p: float, r: float):
    """The header's per-sample step.  Returns (iter, r2, lastZ x, lastZ y, rebases): iter = the loop index of the escaping
    update (max_iter if none), r2 = |z|^2 there (0 for interior), lastZ = z there (interior: Z_m + dz of the final state, which
    is the z of the last update)."""
    ox, oy = np.ascontiguousarray(orbit[:, 0]), np.ascontiguousarray(orbit[:, 1])
    N = len(orbit) - 1
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
    rebases = 0
    for i in range(max_iter):
        if idx.size == 0:
            break
        Zx, Zy = ox[m], oy[m]
        tx = ((Zx + Zx) + dzx) + p
        ty = (Zy + Zy) + dzy
        nx = ((tx * dzx - ty * dzy) + r * dqx) + cx
        ny = ((tx * dzy + ty * dzx) + r * dqy) + cy
        dqx, dqy = dzx, dzy
        m = m + 1
        zx, zy = ox[m] + nx, oy[m] + ny
        qx, qy = ox[m - 1] + dqx, oy[m - 1] + dqy
        r2 = zx * zx + zy * zy
        esc = r2 > four
        small = (r2 + rr * (qx * qx + qy * qy)) < ((nx * nx + ny * ny) + rr * (dqx * dqx + dqy * dqy))
        reb = ~esc & (small | (m == N))
        rebases += int(reb.sum())
        dzx = np.where(reb, zx, nx); dzy = np.where(reb, zy, ny)
        dqx = np.where(reb, qx, dqx); dqy = np.where(reb, qy, dqy)
        m = np.where(reb, 0, m)
        if esc.any():
            e = idx[esc]
            it[e] = i
            r2out[e] = r2[esc]
            ezx[e] = zx[esc]; ezy[e] = zy[esc]
            k = ~esc
            idx, dzx, dzy, dqx, dqy, m, cx, cy = idx[k], dzx[k], dzy[k], dqx[k], dqy[k], m[k], cx[k], cy[k]
    ezx[idx] = ox[m] + dzx; ezy[idx] = oy[m] + dzy           # lastZ of a sample that never escaped: Z_m + dz of its final state
    return it.reshape(shape), r2out.reshape(shape), ezx.reshape(shape), ezy.reshape(shape), rebases


def view_orbit(view: dict) -> np.ndarray:
    return reference_orbit(view["cx"], view["cy"], view["zoom"], view["max_iter"], view["p"], view["r"])


def samples(view: dict, W: int, H: int, aa: int = 1, rows=None, orbit=None):
    """Every sub-sample of the frame (or of its rows), sx outer: a list over s of (iter, r2, lastZ x, lastZ y) planes, and the
    rebases over all of them"""
    if orbit is None:
        orbit = view_orbit(view)
    n_aa = max(int(aa), 1)
    out, rebases = [], 0
    for s in range(n_aa * n_aa):
        dcx, dcy = S.sample_dc(W, H, view["zoom"], n_aa, s, rows)
        it, r2, ezx, ezy, rb = perturb(orbit, dcx, dcy, view["max_iter"], view["p"], view["r"])
        out.append((it, r2, ezx, ezy))
        rebases += rb
    return out, rebases


def smooth(it: np.ndarray, ezx: np.ndarray, ezy: np.ndarray, max_iter: int) -> np.ndarray:
    """nu of the fp64 Phoenix path: i + 1 - log(log|z|^2 / 2 / ln 2) / ln 2 of lastZ, max_iter for interior"""
    return PH.smooth_of(it.ravel(), ezx.ravel(), ezy.ravel(), max_iter, np.float64).reshape(it.shape)


def colour(smp: list, max_iter: int, density: float = 0.0, post: bool = False, brightness: float = 1.0, saturation: float = 1.0,
           contrast: float = 1.0) -> np.ndarray:
    """rgb of samples(): the fp64 Phoenix path's colour stage on each sub-sample, the average in the kernel's order (from a
    zero accumulator), then on request the post chain with Phoenix's floors"""
    acc = np.zeros(smp[0][0].shape + (3,), F32)
    for it, _, ezx, ezy in smp:
        sm = smooth(it, ezx, ezy, max_iter)
        with np.errstate(invalid="ignore"):
            t = (sm / np.float64(max_iter)).astype(F32)
            acc = acc + PH.colour(t, sm.astype(F32), ezx.astype(F32), ezy.astype(F32), density)
    rgb = acc / F32(len(smp))
    return PH.post_chain(rgb, brightness, saturation, contrast) if post else rgb


def restate(view: dict, W: int, H: int, aa: int = 1, density: float = 0.0, post: bool = False, rows=None, orbit=None):
    """A frame (or its rows): (iter, nu, rgb, r2, rebases) -- iter / nu / r2 of sample (0,0), rgb of all of them"""
    smp, rebases = samples(view, W, H, aa, rows, orbit)
    it, r2, ezx, ezy = smp[0]
    return it, smooth(it, ezx, ezy, view["max_iter"]), colour(smp, view["max_iter"], density, post), r2, rebases


def exact_iter(view: dict, x: int, y: int, W: int, H: int, aa: int = 1, s: int = 0, F: int = 0) -> int:
    """The escape index of one sample by the direct iteration of the recurrence in fixed point at F + 64 fraction bits,
    c = centre + dc exactly (then rounded once); p and r exactly"""
    G = (F or R.frac_bits(view["zoom"])) + 64
    dcx, dcy = S.sample_dc(W, H, view["zoom"], aa, s, rows=[y])
    cr = round((Fraction(view["cx"]) + Fraction(float(dcx[0, x]))) * (1 << G))
    ci = round((Fraction(view["cy"]) + Fraction(float(dcy[0, x]))) * (1 << G))
    P, Rr = _fixed_floor(view["p"], G), _fixed_floor(view["r"], G)
    T = 4 << (2 * G)
    zr = zi = qr = qi = 0
    for i in range(view["max_iter"]):
        nr = ((zr * zr - zi * zi + Rr * qr + P * zr) >> G) + cr
        ni = ((2 * zr * zi + Rr * qi + P * zi) >> G) + ci
        qr, qi, zr, zi = zr, zi, nr, ni
        if zr * zr + zi * zi > T:
            return i
    return view["max_iter"]


def exact_frame(view: dict, W: int, H: int) -> np.ndarray:
    """exact_iter of every pixel's sample (0,0), aa 1"""
    return np.array([[exact_iter(view, x, y, W, H) for x in range(W)] for y in range(H)], np.int32)
