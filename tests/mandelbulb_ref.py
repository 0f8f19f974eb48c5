"""numpy restatement of shaders/mandelbulb.comp in fp32, vectorised over samples.

Every operation is a numpy float32 operation in the order the SPIR-V interpreter (tests/golden/spirv_interp_ext.py)
executes the compiled shader, with the same numpy functions for the transcendentals, so on one host it reproduces the
fixture tests/golden/mandelbulb_spv_frames.npz (tests/test_mandelbulb_host.py pins how closely).  GLSL max / clamp
follow the interpreter's operand order (FMax: x < y ? y : x; FClamp: min(max(x, lo), hi)), which keeps NaN: the linear
colour carries the shader's NaN; post_chain() maps NaN to 0 as the library's post chain does.

render(W, H, **params) -> (iter, t, rgb_linear) for sample (0,0) of every pixel (iter: hit step, -1 for a miss) and the
averaged linear colour; rows=(r0, r1) restricts it to a band of rows.  de_calls counts the DE evaluations of the most
recent render (tools/mandelbulb_time.py reports the rate).
"""
import numpy as np

F = np.float32
LIGHT = np.array([0x3f1d8e9f, 0x3f1d8e9f, 0x3efc1764], np.uint32).view(np.float32)   # normalize(vec3(1, 1, 0.8))
GAMMA = np.array([0x3ee8ba2f], np.uint32).view(np.float32)[0]                         # 1.0 / 2.2
DEFAULTS = dict(camera_distance=3.0, rotation_y=0.0, fov=1.0, mandelbulb_power=8.0, rotation_speed=0.5, time=0.0,
                max_iterations=256, aa=1, palette_mode=0, color_offset=0.0, color_scale=1.0, color_brightness=1.0,
                color_saturation=1.0, color_contrast=1.0)
de_calls = 0


def _max(x, y):
    return np.where(x < y, y, x).astype(F)


def _clamp(x, lo, hi):
    m = np.where(F(lo) > x, F(lo), x)
    return np.where(F(hi) < m, F(hi), m).astype(F)


def _fract(x):
    return (x - np.floor(x)).astype(F)


def _mix(x, y, a):
    return x * (F(1.0) - a) + y * a


def de(px, py, pz, power, max_iter):
    """mandelbulb_de (:96-108) for arrays of points: (distance, escape_iter)"""
    global de_calls
    de_calls += px.size
    n = px.size
    zx, zy, zz = px.copy(), py.copy(), pz.copy()
    dr = np.ones(n, F)
    r = np.zeros(n, F)
    esc = np.full(n, F(max_iter), F)
    act = np.arange(n)
    pw1 = F(power - F(1.0))
    for i in range(max_iter):
        if act.size == 0:
            break
        x, y, z = zx[act], zy[act], zz[act]
        rr = np.sqrt((x * x + y * y) + z * z)
        r[act] = rr
        out = rr > F(2.0)
        esc[act[out]] = F(i)
        keep = ~out & ~(rr < F(0.0001))
        act, x, y, z, rr = act[keep], x[keep], y[keep], z[keep], rr[keep]
        theta = np.arccos(_clamp(z / rr, -1.0, 1.0))
        phi = np.arctan2(y, x)
        r_pow = np.power(rr, pw1)
        dr[act] = (r_pow * power) * dr[act] + F(1.0)
        zr = np.power(rr, power)
        theta = theta * power
        phi = phi * power
        st, ct, sp, cp = np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi)
        zx[act] = (st * cp) * zr + px[act]
        zy[act] = (sp * st) * zr + py[act]
        zz[act] = ct * zr + pz[act]
    d = ((F(0.5) * np.log(r)) * r) / dr
    d = np.where((r < F(0.0001)) | (dr < F(0.0001)), F(0.0), d).astype(F)
    return d, esc


def _hash(x, y):
    return _fract(np.sin(x * F(127.1) + y * F(311.7)) * F(43758.5453123))


def _noise(px, py):
    ix, iy = np.floor(px), np.floor(py)
    fx, fy = _fract(px), _fract(py)
    a, b = _hash(ix, iy), _hash(ix + F(1.0), iy + F(0.0))
    c, d = _hash(ix + F(0.0), iy + F(1.0)), _hash(ix + F(1.0), iy + F(1.0))
    ux, uy = (fx * fx) * (F(3.0) - F(2.0) * fx), (fy * fy) * (F(3.0) - F(2.0) * fy)
    return (_mix(a, b, ux) + ((c - a) * uy) * (F(1.0) - ux)) + ((d - b) * ux) * uy


def _hsv2rgb(h, s, v):
    out = []
    for off in (0.0, 4.0, 2.0):
        x = h * F(6.0) + F(off)
        m = x - F(6.0) * np.floor(x / F(6.0))
        c = _clamp(np.abs(m - F(3.0)) - F(1.0), 0.0, 1.0)
        out.append(_mix(F(1.0), c, s) * v)
    return out


def _dynamic(t):
    hue = _fract(t + F(0.3) * np.sin(t * F(12.0)))
    sat = F(0.6) + F(0.4) * np.sin(t * F(7.0))
    return _hsv2rgb(hue, sat, np.power(t, F(0.4)))


def _fire_ice(t):
    s = _clamp((t - F(0.0)) / (F(1.0) - F(0.0)), 0.0, 1.0)
    blend = (s * s) * (F(3.0) - F(2.0) * s)
    f = _fract(t * F(3.0))
    return [_mix(np.power(blend, F(2.0)), F(0.0), f), _mix(blend * F(0.5), F(0.5) + F(0.5) * blend, f), _mix(F(0.0), F(1.0), f)]


_LAVA = np.array([[0.1, 0.0, 0.0], [0.8, 0.1, 0.0], [1.0, 0.5, 0.0], [1.0, 0.9, 0.3], [1.0, 1.0, 0.8]], F)


def _lava(t):
    seg = np.where(t < F(0.25), 0, np.where(t < F(0.5), 1, np.where(t < F(0.75), 2, 3)))
    w = np.where(seg == 0, t * F(4.0), np.where(seg == 1, (t - F(0.25)) * F(4.0),
                 np.where(seg == 2, (t - F(0.5)) * F(4.0), (t - F(0.75)) * F(4.0)))).astype(F)
    return [_mix(_LAVA[seg, k], _LAVA[seg + 1, k], w) for k in range(3)]


def _neon(t):
    c1, c2, c3, c4 = (0.0, 0.0, 0.1), (0.0, 0.2, 0.6), (0.0, 0.8, 1.0), (0.5, 1.0, 1.0)
    w = np.power(t, F(2.0))
    return [_mix(_mix(F(c1[k]), F(c2[k]), t), _mix(F(c3[k]), F(c4[k]), t), w) for k in range(3)]


def palette(t, mode):
    """get_palette_color, :63-75 (mode in [0, 5], one mode for the whole array)"""
    t = _fract(t)
    n = _noise(t * F(100.0), t * F(57.0)) * F(0.02)
    if mode == 4:
        t = np.power(t, F(0.5))
    elif mode == 5:
        t = np.power(t, F(0.6))
    x = t + n
    return {0: _dynamic, 4: _dynamic, 1: _fire_ice, 5: _fire_ice, 2: _lava, 3: _neon}[mode](x)


def _shade(px, py, pz, rd, t, d, esc, power, max_iter, c_off, c_scale, mode, mix_w):
    """the hit branch of raymarch, :142-160"""
    eps = F(0.001)
    d0, _ = de(px, py, pz, power, max_iter)
    nx = de(px + eps, py + F(0.0), pz + F(0.0), power, max_iter)[0] - d0
    ny = de(px + F(0.0), py + eps, pz + F(0.0), power, max_iter)[0] - d0
    nz = de(px + F(0.0), py + F(0.0), pz + eps, power, max_iter)[0] - d0
    ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
    small = ln < F(0.0001)
    with np.errstate(all="ignore"):
        nx, ny, nz = np.where(small, F(0.0), nx / ln), np.where(small, F(1.0), ny / ln), np.where(small, F(0.0), nz / ln)
    nx, ny, nz = nx.astype(F), ny.astype(F), nz.astype(F)
    lx, ly, lz = LIGHT
    diffuse = _max((nx * lx + ny * ly) + nz * lz, F(0.0))
    vx, vy, vz = -rd[0], -rd[1], -rd[2]
    ix, iy, iz = -lx, -ly, -lz
    k2 = F(2.0) * ((nx * ix + ny * iy) + nz * iz)
    fx, fy, fz = ix - k2 * nx, iy - k2 * ny, iz - k2 * nz
    spec = np.power(_max((vx * fx + vy * fy) + vz * fz, F(0.0)), F(64.0))
    rim = np.power(F(1.0) - _max((nx * vx + ny * vy) + nz * vz, F(0.0)), F(2.0))
    glow, fglow = np.exp(F(-8.0) * d), np.exp(F(-30.0) * d)
    lp = np.sqrt((px * px + py * py) + pz * pz)
    it = (esc + F(1.0)) - np.log(np.log(lp)) / np.log(power + F(0.0001))
    it = it / F(max_iter)
    it = _fract(c_off + np.power(it, F(0.6)) * c_scale)
    base = palette(it, mode)
    alt = palette(_fract(it + F(0.33)), (mode + 1) % 6)
    light = F(0.15) + diffuse * F(0.9)
    ao = np.zeros_like(px)
    k = F(0.01)
    n_ao = 0
    while k < F(0.15):                                   # 8 passes in float
        e, _ = de(nx * k + px, ny * k + py, nz * k + pz, power, max_iter)
        ao = ao + np.exp(F(-10.0) * e)
        k = F(k + F(0.02))
        n_ao += 1
    assert n_ao == 8
    ao = F(1.0) - ao / F(8.0)
    occl = ao * F(0.8) + F(0.2)
    fog = _clamp(t / F(10.0), 0.0, 1.0) * F(0.6)
    out = []
    for c, (fg, sk) in enumerate(((1.0, 0.0), (0.8, 0.0), (0.5, 0.1))):
        v = _mix(base[c], alt[c], mix_w)
        v = v * light
        v = v + spec * F(0.5)
        v = v + rim * F(0.25)
        v = v + glow * F(0.5)
        v = v + (F(fg) * fglow) * F(0.5)
        v = v * occl
        out.append(_mix(v, F(sk), fog))
    return out


def camera(p):
    """main's clamps and camera (:177-209): a dict of the per-frame values"""
    f = lambda k: F(p[k])   # noqa: E731
    cd = _max(f("camera_distance"), F(0.1))
    power = _clamp(f("mandelbulb_power"), 2.0, 16.0)
    max_iter = int(min(max(int(p["max_iterations"]), 1), 1024))
    c_scale = _max(f("color_scale"), F(0.1))
    mode = int(min(max(int(p["palette_mode"]), 0), 5))
    time = f("time")
    fov = _clamp(f("fov"), 0.1, 3.0)
    aa = max(int(p["aa"]), 1)
    rs = f("rotation_speed")
    rs = rs if rs != F(0.0) else F(0.3)
    rot = f("rotation_y") + rs * time
    dist = cd * (F(1.0) + F(0.3) * np.sin(time * F(0.5)))
    c, s = np.cos(rot), np.sin(rot)
    ro = ((c * F(0.0) + F(0.0) * F(0.0)) + (-s) * dist, (F(0.0) * F(0.0) + F(1.0) * F(0.0)) + F(0.0) * dist,
          (s * F(0.0) + F(0.0) * F(0.0)) + c * dist)
    fw = [-ro[0], -ro[1], -ro[2]]
    ln = np.sqrt((fw[0] * fw[0] + fw[1] * fw[1]) + fw[2] * fw[2])
    fw = [v / ln for v in fw]
    rt = [F(1.0) * fw[2] - fw[1] * F(0.0), F(0.0) * fw[0] - fw[2] * F(0.0), F(0.0) * fw[1] - fw[0] * F(1.0)]
    ln = np.sqrt((rt[0] * rt[0] + rt[1] * rt[1]) + rt[2] * rt[2])
    rt = [v / ln for v in rt]
    up = [fw[1] * rt[2] - rt[1] * fw[2], fw[2] * rt[0] - rt[2] * fw[0], fw[0] * rt[1] - rt[0] * fw[1]]
    return dict(ro=ro, fw=fw, rt=rt, up=up, fov=fov, power=F(power + F(0.5) * np.sin(time * F(0.7))), max_iter=max_iter,
                c_off=f("color_offset"), c_scale=c_scale, mode=mode, aa=aa, mix_w=F(0.3) + F(0.3) * np.sin(time * F(0.5)),
                brightness=_max(f("color_brightness"), F(0.1)), saturation=_max(f("color_saturation"), F(0.0)),
                contrast=_max(f("color_contrast"), F(0.1)))


def march(cam, px, py, sx, sy, W, H):
    """one sample per element: (rgb list, hit step or -1, t where the march stopped)"""
    aa = F(cam["aa"])
    ux = ((px.astype(F) + F(sx) / aa) - F(W) * F(0.5)) / F(H)
    uy = ((py.astype(F) + F(sy) / aa) - F(H) * F(0.5)) / F(H)
    fw, rt, up, fov, ro = cam["fw"], cam["rt"], cam["up"], cam["fov"], cam["ro"]
    rd = [(fw[k] + (rt[k] * ux) * fov) + (up[k] * uy) * fov for k in range(3)]
    ln = np.sqrt((rd[0] * rd[0] + rd[1] * rd[1]) + rd[2] * rd[2])
    rd = [v / ln for v in rd]
    n = px.size
    t = np.full(n, F(0.001), F)
    step = np.full(n, -1, np.int32)
    hit_d = np.zeros(n, F)
    hit_e = np.zeros(n, F)
    act = np.arange(n)
    for i in range(200):
        if act.size == 0:
            break
        tt = t[act]
        pos = [rd[k][act] * tt + ro[k] for k in range(3)]
        d, esc = de(pos[0], pos[1], pos[2], cam["power"], cam["max_iter"])
        bad = np.isnan(d) | np.isinf(d)
        thr = _max(F(0.0001), F(0.001) * tt)
        hit = ~bad & (d < thr)
        step[act[hit]] = i
        hit_d[act[hit]] = d[hit]
        hit_e[act[hit]] = esc[hit]
        stop = bad | hit | (tt > F(10.0)) | (d > F(10.0))
        go = ~stop
        t[act[go]] = tt[go] + _max(d[go] * F(0.5), F(0.0005))
        act = act[go]
    sky = _clamp(rd[1] * F(0.5) + F(0.5), 0.0, 1.0)
    rgb = [_mix(F(lo), F(hi), sky) for lo, hi in ((0.02, 0.5), (0.02, 0.6), (0.05, 0.8))]
    h = np.nonzero(step >= 0)[0]
    if h.size:
        th = t[h]
        pos = [rd[k][h] * th + ro[k] for k in range(3)]
        col = _shade(pos[0], pos[1], pos[2], [rd[k][h] for k in range(3)], th, hit_d[h], hit_e[h], cam["power"],
                     cam["max_iter"], cam["c_off"], cam["c_scale"], cam["mode"], cam["mix_w"])
        for k in range(3):
            rgb[k][h] = col[k]
    return rgb, step, t


def render(W, H, rows=None, **params):
    global de_calls
    de_calls = 0
    p = dict(DEFAULTS)
    p.update(params)
    r0, r1 = rows or (0, H)
    with np.errstate(all="ignore"):
        cam = camera(p)
        py, px = np.mgrid[r0:r1, 0:W]
        px, py = px.ravel(), py.ravel()
        acc = [np.zeros(px.size, F) for _ in range(3)]
        aa = cam["aa"]
        for sy in range(aa):
            for sx in range(aa):
                rgb, step, t = march(cam, px, py, sx, sy, W, H)
                if sx == 0 and sy == 0:
                    it0, t0 = step, t
                acc = [acc[k] + rgb[k] for k in range(3)]
        nn = F(aa * aa)
        lin = np.stack([a / nn for a in acc], axis=-1).astype(F)
    shape = (r1 - r0, W)
    return it0.reshape(shape), t0.reshape(shape), lin.reshape(shape + (3,))


def post_chain(lin, brightness=1.0, saturation=1.0, contrast=1.0):
    """enhance_color -> aces_tonemap -> pow(1/2.2) with main's floors (:187-190); NaN -> 0 at enhance_color's clamp"""
    with np.errstate(all="ignore"):
        b, s, c = _max(F(brightness), F(0.1)), _max(F(saturation), F(0.0)), _max(F(contrast), F(0.1))
        x = lin.astype(F) * b
        x = (x - F(0.5)) * c + F(0.5)
        gray = (x[..., 0] * F(0.299) + x[..., 1] * F(0.587)) + x[..., 2] * F(0.114)
        x = _mix(gray[..., None], x, s)
        x = np.minimum(np.maximum(np.nan_to_num(x, nan=0.0), F(0.0)), F(1.0)).astype(F)
        a = (x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))
        a = np.minimum(np.maximum(a, F(0.0)), F(1.0))
        return np.power(a, GAMMA).astype(F)


def post_chain_as_interpreted(lin, brightness=1.0, saturation=1.0, contrast=1.0):
    """the same chain with the interpreter's clamp, which keeps NaN (what the fixture's rgba holds)"""
    with np.errstate(all="ignore"):
        b, s, c = _max(F(brightness), F(0.1)), _max(F(saturation), F(0.0)), _max(F(contrast), F(0.1))
        x = lin.astype(F) * b
        x = (x - F(0.5)) * c + F(0.5)
        gray = (x[..., 0] * F(0.299) + x[..., 1] * F(0.587)) + x[..., 2] * F(0.114)
        x = _clamp(_mix(gray[..., None], x, s), 0.0, 1.0)
        a = _clamp((x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14)), 0.0, 1.0)
        return np.power(a, GAMMA).astype(F)
