"""Vectorised numpy restatement of shaders/phoenix.comp (fr_render_phoenix), in fp32 and fp64.

TEST INFRASTRUCTURE ONLY.  Pinned to the reference by tests/golden/phoenix_spv_frames.npz (the reference's compiled
shader executed by tests/golden/spirv_interp.py); the checker of the GPU kernels at sizes the interpreter cannot reach.
numpy performs one IEEE operation per ufunc call, in the order written here, so no contraction can occur.

Semantics (shaders/phoenix.comp:34-168):
  map        uv = pix / size (+ the supersampling offset, divided by size AGAIN), c = centre + ((uv.x - 0.5) * zoom * aspect,
             (uv.y - 0.5) * zoom), aspect = W / H                                                       (:103-110, :157)
  loop       z = prev = 0; x = (((zx*zx - zy*zy) + C.x) + r*prev.x) + p*zx, y = ((((2*zx)*zy) + C.y) + r*prev.y) + p*zy;
             prev = z; z = (x, y); break when zx^2 + zy^2 > 4 (update, then test); C = julia_c in Julia mode  (:63-79)
  smooth     i + 1 - log(log(|z|^2)/2 / log 2) / log 2; interior: float(max_iter)                          (:80-83)
  colour     t = pow(smooth / max_iter, 0.8) through ultra_fire (palette_mode ignored), flow stripes when
             max(density, 0) > 0.01                                                                     (:119-140)
fp64: map, orbit and smooth in double; t = smooth / max_iter divided in double and narrowed, the colour stage in float.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
_C = np.array([[0.0, 0.0, 0.1], [0.8, 0.0, 0.0], [1.0, 0.3, 0.0], [1.0, 0.9, 0.0], [1.0, 1.0, 0.95]], F32)   # :19-23


def _fract(x):
    return x - np.floor(x)


def fire(t):
    """get_palette_color -> palette_ultra_fire, :18-43 (float32 in, (..., 3) float32 out).  NaN takes c5."""
    t = _fract(t.astype(F32))
    t = np.power(t, F32(0.7))
    five = F32(5.0)
    segs = [(t < F32(0.2), 0, t * five), (t < F32(0.4), 1, (t - F32(0.2)) * five),
            (t < F32(0.6), 2, (t - F32(0.4)) * five), (t < F32(0.8), 3, (t - F32(0.6)) * five)]
    out = np.broadcast_to(_C[4], t.shape + (3,)).copy()
    done = np.zeros(t.shape, bool)
    for cond, k, w in segs:
        sel = cond & ~done
        w3 = w[..., None]
        mix = _C[k] * (F32(1.0) - w3) + _C[k + 1] * w3
        out[sel] = mix[sel]
        done |= cond
    return out


def colour(t, smooth, ezx, ezy, density):
    """:119-140 in float32: t = smooth / max_iter (before the pow), smooth, lastZ narrowed."""
    t = np.power(t.astype(F32), F32(0.8))
    dens = max(F32(density), F32(0.0))
    if not dens > F32(0.01):
        return fire(t)
    amp = F32(min(max(dens * F32(0.05), F32(0.0)), F32(1.0)))
    smooth = smooth.astype(F32)
    angle = np.arctan2(ezy.astype(F32), ezx.astype(F32))
    mod = F32(0.5) + F32(0.5) * np.sin(angle * dens + smooth * F32(0.25))
    adaptive = amp * (F32(1.0) - np.exp(F32(-0.004) * smooth * smooth))
    t2 = _fract(t + F32(0.1) * mod)
    w = (adaptive * mod)[..., None]
    return fire(t) * (F32(1.0) - w) + fire(t2) * w


def post_chain(rgb, brightness=1.0, saturation=1.0, contrast=1.0):
    """enhance_color -> aces_tonemap -> pow(1/2.2) with Phoenix's floors, :47-58, :160-166"""
    b = max(F32(brightness), F32(0.1))
    s = max(F32(saturation), F32(0.0))
    k = max(F32(contrast), F32(0.1))
    c = rgb.astype(F32) * b
    c = (c - F32(0.5)) * k + F32(0.5)
    gray = (c[..., 0] * F32(0.299) + c[..., 1] * F32(0.587) + c[..., 2] * F32(0.114))[..., None]
    c = np.clip(gray * (F32(1.0) - s) + c * s, F32(0.0), F32(1.0))
    a, bb, cc, d, e = F32(2.51), F32(0.03), F32(2.43), F32(0.59), F32(0.14)
    c = np.clip((c * (a * c + bb)) / (c * (cc * c + d) + e), F32(0.0), F32(1.0))
    return np.power(c, F32(1.0 / 2.2))


def orbit(cx, cy, p, r, max_iter, T):
    """phoenix_iter's loop for arrays of C: (escape index i or max_iter, lastZ x, lastZ y)."""
    n = cx.size
    it = np.full(n, max_iter, np.int32)
    ezx = np.zeros(n, T)
    ezy = np.zeros(n, T)
    idx = np.arange(n)
    zx = np.zeros(n, T); zy = np.zeros(n, T); qx = np.zeros(n, T); qy = np.zeros(n, T)
    cx = cx.astype(T).copy(); cy = cy.astype(T).copy()
    p, r, two, four = T(p), T(r), T(2.0), T(4.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(max_iter):
            if idx.size == 0:
                break
            x = (((zx * zx - zy * zy) + cx) + r * qx) + p * zx
            y = ((((two * zx) * zy) + cy) + r * qy) + p * zy
            qx, qy, zx, zy = zx, zy, x, y
            esc = (zx * zx + zy * zy) > four
            if esc.any():
                e = idx[esc]
                it[e] = i
                ezx[e] = zx[esc]
                ezy[e] = zy[esc]
                keep = ~esc
                idx, zx, zy, qx, qy, cx, cy = idx[keep], zx[keep], zy[keep], qx[keep], qy[keep], cx[keep], cy[keep]
    ezx[idx] = zx
    ezy[idx] = zy
    return it, ezx, ezy


def smooth_of(it, ezx, ezy, max_iter, T):
    d = ezx * ezx + ezy * ezy
    ln2 = np.log(T(2.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        log_zn = np.log(d) / T(2.0)
        nu = np.log(log_zn / ln2) / ln2
        sm = (it.astype(T) + T(1.0)) - nu
    return np.where(it < max_iter, sm, T(max_iter)).astype(T)


def render(W, H, *, center_x=-0.5, center_y=0.0, zoom=3.0, max_iterations=256, julia_c_real=float(F32(-0.7)),
           julia_c_imag=float(F32(0.27015)), phoenix_p=0.0, phoenix_r=-0.5, use_julia_set=False, aa=1,
           stripe_density=10.0, color_brightness=1.0, color_saturation=1.0, color_contrast=1.0, post=False,
           f64=False, rows=None):
    """One frame (or the rows `rows` of it).  Returns (iter, smooth, rgb): iter / smooth of sample (0,0) of every pixel,
    rgb the linear colour (post=True: post-chained), shapes (R, W), (R, W), (R, W, 3)."""
    T = np.float64 if f64 else F32
    rows = np.arange(H) if rows is None else np.asarray(rows)
    px, py = np.meshgrid(np.arange(W), rows)
    max_iter = int(max_iterations)
    n_aa = max(int(aa), 1)
    sizex, sizey = T(W), T(H)
    if f64:
        ctr_x, ctr_y, zm, jx, jy = T(center_x), T(center_y), T(zoom), T(julia_c_real), T(julia_c_imag)
    else:
        ctr_x, ctr_y, zm, jx, jy = F32(center_x), F32(center_y), F32(zoom), F32(julia_c_real), F32(julia_c_imag)
    p, r = T(F32(phoenix_p)), T(F32(phoenix_r))
    aspect = sizex / sizey
    so = (T(1.0) / sizex) / T(n_aa)
    centre_off = so * T(n_aa - 1) * T(0.5)
    base_u = px.astype(T) / sizex
    base_v = py.astype(T) / sizey
    acc = np.zeros(px.shape + (3,), F32)
    it0 = sm0 = None
    for sx in range(n_aa):
        for sy in range(n_aa):
            u = base_u + (T(sx) * so - centre_off) / sizex
            v = base_v + (T(sy) * so - centre_off) / sizey
            cx = ctr_x + ((u - T(0.5)) * zm) * aspect
            cy = ctr_y + (v - T(0.5)) * zm
            if use_julia_set:
                cx = np.full_like(cx, jx)
                cy = np.full_like(cy, jy)
            it, ezx, ezy = orbit(cx.ravel(), cy.ravel(), p, r, max_iter, T)
            sm = smooth_of(it, ezx, ezy, max_iter, T)
            if sx == 0 and sy == 0:
                it0, sm0 = it.reshape(px.shape), sm.reshape(px.shape)
            with np.errstate(invalid="ignore"):
                t = (sm / T(max_iter)).astype(F32)
                rgb = colour(t, sm.astype(F32), ezx.astype(F32), ezy.astype(F32), stripe_density)
            acc = acc + rgb.reshape(px.shape + (3,))
    rgb = acc / F32(n_aa * n_aa)
    if post:
        rgb = post_chain(rgb, color_brightness, color_saturation, color_contrast)
    return it0, sm0, rgb
