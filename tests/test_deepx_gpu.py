"""Deep views with extended-exponent deltas on the GPU (fr_render_deepx): byte-identical to fr_render_deep where no delta
needs the extended mode, against the numpy restatement of the two-mode step (tests/deepx_ref.py) and the direct
fixed-point iteration below the double range, shards, layouts, memory kinds, the asynchronous form and the orbit caches
of one context."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_ref as R
import deepx_ref as X
from test_deep_gpu import NU_TOL, RGB_TOL, _few

pytestmark = pytest.mark.gpu

W, H = 256, 192
V = X.views()
E_ROWS = list(range(84, 108))          # view E: the restatement of a band of rows (8124 steps per sample)


def _xview(name):
    """a view of deep_ref (double zoom) or of deepx_views.json as a deepx view: the zoom a string"""
    if name in V:
        return V[name]
    v = R.VIEWS[name]
    return dict(cx=v["cx"], cy=v["cy"], zoom=repr(v["zoom"]), max_iter=v["max_iter"])


def _render_x(fr, r, v, aa=1, post=False, shard=None, w=W, h=H, **kw):
    rows = shard.rows(h) if shard else h
    rgba = np.empty((rows, w, 4), np.float32)
    nu = np.empty((rows, w), np.float64)
    it = np.empty((rows, w), np.int32)
    r.render_deep(fr.FractalState(max_iterations=v["max_iter"], antialiasing_samples=aa), w, h,
                  fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"]), post_chain=post, rgba=rgba, nu=nu, iter=it, shard=shard, **kw)
    return rgba, nu, it


def _render_plain(fr, r, v, aa=1, post=False, w=W, h=H):
    rgba = np.empty((h, w, 4), np.float32)
    nu = np.empty((h, w), np.float64)
    it = np.empty((h, w), np.int32)
    r.render_deep(fr.FractalState(zoom=float(v["zoom"]), max_iterations=v["max_iter"], antialiasing_samples=aa), w, h,
                  fr.DeepView(v["cx"], v["cy"]), post_chain=post, rgba=rgba, nu=nu, iter=it)
    return rgba, nu, it


@functools.lru_cache(maxsize=None)
def _restated(name, aa, rows=None):
    stats = {}
    return X.restate_x(V[name], W, H, aa, rows=None if rows is None else list(rows), stats=stats), stats


def _expected_rgba(oracle, v, samples, aa, post):
    """test_deep_gpu's colour stage (it does not read the zoom) on the restated samples"""
    p = oracle.OracleParams(max_iterations=v["max_iter"], zoom=1.0, aa=aa, post_chain=0)
    shape = samples[0][0].shape
    acc = np.zeros(shape + (3,), np.float32)
    for it, r2 in samples:
        acc = acc + oracle.colorize(p, R.smooth(it, r2, v["max_iter"]))[..., :3]
    if aa > 1:
        acc = acc / np.float32(aa * aa)
    if post:
        acc = np.array([oracle.post_chain(c) for c in acc.reshape(-1, 3)], np.float32).reshape(shape + (3,))
    return acc


def _check_planes(oracle, v, got, samples, aa, post):
    rgba, nu, it = got
    r_it, r_r2 = samples[0]
    ndiff = int((it != r_it).sum())
    dnu = float(np.abs(nu - R.smooth(r_it, r_r2, v["max_iter"])).max())
    bad = np.abs(rgba[..., :3] - _expected_rgba(oracle, v, samples, aa, post)).max(axis=2) > RGB_TOL
    print("iter differences", ndiff, "max |nu - restated|", dnu, "rgb outside tolerance", int(bad.sum()), "of", it.size)
    assert ndiff == 0
    assert dnu <= NU_TOL
    assert np.all(rgba[..., 3] == 1.0)
    assert _few(bad, it.size), int(bad.sum())


def _check_exact(name, it):
    g = X.exact_golden()
    ex, ys, xs = g[name], g["ys"], g["xs"]
    share = float(np.unique(ex, return_counts=True)[1].max()) / len(ex)
    agree = float((it[ys, xs] == ex).mean())
    print(name, "largest share of one exact count", share, "agreement with the exact iteration", agree)
    assert share <= 0.60                                           # a collapsed frame cannot agree by chance
    assert agree >= 0.99
    for k in (3, 200):                                             # the fixture is exact_iter_x: two samples live
        if name != "E":
            assert X.exact_iter_x(V[name], int(xs[k]), int(ys[k]), W, H) == ex[k]


# 1. where no delta needs the extended mode the new entry writes the bytes of fr_render_deep
@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("aa", [1, 2])
@pytest.mark.parametrize("name", ["A", "B"])
def test_shallow_views_are_byte_identical_to_fr_render_deep(fr, renderer, name, aa, post):
    v = _xview(name)
    got = _render_x(fr, renderer, v, aa, post)
    want = _render_plain(fr, renderer, v, aa, post)
    for g, w_ in zip(got, want):
        assert np.array_equal(g.view(np.uint8), w_.view(np.uint8))


# 2. below the double range
@pytest.mark.parametrize("name,aa,post", [("D", 1, False), ("D", 2, True), ("E", 1, True)])
def test_views_below_the_double_range_match_the_restatement(fr, renderer, oracle, name, aa, post):
    v = V[name]
    got = _render_x(fr, renderer, v, aa, post)
    rows = tuple(E_ROWS) if name == "E" else None
    samples, stats = _restated(name, aa, rows)
    print(name, stats)
    assert stats["ext_steps"] > stats["plain_steps"] and stats["to_plain"] > 0
    if rows is not None:
        got = tuple(p[E_ROWS] for p in got)
    _check_planes(oracle, v, got, samples, aa, post)


@pytest.mark.parametrize("name", ["D", "E"])
def test_views_below_the_double_range_agree_with_the_exact_iteration(fr, renderer, name):
    _, _, it = _render_x(fr, renderer, V[name])
    _check_exact(name, it)


# 3. either side of the mode threshold (2^-400: T110 / T130) and of the double range (T260 .. T320)
@pytest.mark.parametrize("name", ["T110", "T130", "T260", "T280", "T300", "T320"])
def test_views_around_the_thresholds(fr, renderer, oracle, name):
    v = V[name]
    got = _render_x(fr, renderer, v)
    samples, stats = _restated(name, 1)
    print(name, stats)
    if name == "T110":
        assert stats["ext_steps"] <= W * H + v["max_iter"]          # the first step of every sample (and the one with dc = 0)
    else:
        assert stats["ext_steps"] > 10 * W * H and stats["to_plain"] >= W * H - 1
    _check_planes(oracle, v, got, samples, 1, False)
    _check_exact(name, got[2])
    if name == "T280":
        # both entries can render this view; they differ by the roundings of the extended steps only.  The number of iter
        # values that differ is whatever the two restatements give on the CPU -- the GPU must give the same number.
        plain_v = dict(cx=v["cx"], cy=v["cy"], zoom=float(v["zoom"]), max_iter=v["max_iter"])
        cpu = int((R.restate(plain_v, W, H)[0][0][0] != samples[0][0]).sum())
        gpu = int((_render_plain(fr, renderer, v)[2] != got[2]).sum())
        print("T280: iter values that differ between fr_render_deep and fr_render_deepx: restatements", cpu, "GPU", gpu,
              "of", W * H)
        assert gpu == cpu


# 4. shards, layouts, memory kinds, the asynchronous form
def test_shards_layouts_memory_and_async(fr, renderer):
    import torch
    v = V["D"]
    w, h = 203, 117
    ref_rgba, ref_nu, ref_it = _render_x(fr, renderer, v, 2, True, w=w, h=h)
    assert renderer.last_kernel_ms() > 0.0 and renderer.last_grid() > 0
    assert len(np.unique(ref_it)) > 5
    for nparts in (1, 3, 8):
        rgba = np.zeros_like(ref_rgba); nu = np.zeros_like(ref_nu); it = np.full_like(ref_it, -7)
        for part in range(nparts):
            sh = fr.Shard(part, nparts)
            g = sh.global_rows(h)
            a, n, i = _render_x(fr, renderer, v, 2, True, shard=sh, w=w, h=h)
            rgba[g], nu[g], it[g] = a, n, i
        assert np.array_equal(rgba, ref_rgba) and np.array_equal(nu.view(np.uint64), ref_nu.view(np.uint64)) \
            and np.array_equal(it, ref_it), nparts
    dev = torch.device("cuda:0")
    st = fr.FractalState(max_iterations=v["max_iter"], antialiasing_samples=2)
    view = fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"])
    for sync in (True, False):
        d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
        d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
        d_it = torch.zeros((h, w), dtype=torch.int32, device=dev)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        if sync:
            renderer.render_deep(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it)
        else:
            renderer.render_deep(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it,
                                 stream=s.cuda_stream, sync=False)
            s.synchronize()
            renderer.check()
        assert np.array_equal(d_rgba.cpu().numpy(), ref_rgba) and np.array_equal(d_it.cpu().numpy(), ref_it)
        assert np.array_equal(d_nu.cpu().numpy().view(np.uint64), ref_nu.view(np.uint64)), sync
    # FR_LAYOUT_FRAME: each part writes its rows in place into whole-frame device planes
    L = fr.lib()
    p = st.to_params(fr.FractalType.Mandelbrot, fr.Precision.F64, True)
    cv = view.to_cx()
    d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
    d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
    d_it = torch.full((h, w), -7, dtype=torch.int32, device=dev)
    o = fr._capi.fr_output(d_rgba.data_ptr(), d_nu.data_ptr(), d_it.data_ptr(), fr._capi.FR_MEM_DEVICE, fr._capi.FR_LAYOUT_FRAME)
    torch.cuda.synchronize()
    for part in range(3):
        sh = fr._capi.fr_shard(part, 3, 16)
        assert L.fr_render_deepx(renderer._ctx, C.byref(p), C.byref(cv), w, h, C.byref(sh), C.byref(o)) == 0
    assert np.array_equal(d_rgba.cpu().numpy(), ref_rgba) and np.array_equal(d_it.cpu().numpy(), ref_it)
    assert np.array_equal(d_nu.cpu().numpy().view(np.uint64), ref_nu.view(np.uint64))
    # the options that have no effect on it are accepted
    renderer.set_option("periodicity", 1)
    renderer.set_option("staging", 1)
    a, n, i = _render_x(fr, renderer, v, 2, True, w=w, h=h)
    renderer.set_option("periodicity", 0)
    renderer.set_option("staging", 0)
    assert np.array_equal(a, ref_rgba) and np.array_equal(i, ref_it)


# 5. the orbit caches of one context
def test_orbit_caches_do_not_leak_between_paths(fr):
    W2, H2 = 160, 120

    def deepx(r, name):
        return _render_x(fr, r, _xview(name), 1, True, w=W2, h=H2)

    def deep(r, name):
        return _render_plain(fr, r, _xview(name), 1, True, w=W2, h=H2)

    def deep_zoom(r):
        st = fr.FractalState(center_x=-0.743643887037151, center_y=0.131825904205330, zoom=1e-5, max_iterations=512,
                             use_perturbation=True)
        rgba = np.empty((H2, W2, 4), np.float32)
        it = np.empty((H2, W2), np.int32)
        r.render(st, W2, H2, fractal_type=fr.FractalType.Deep_Zoom, precision=fr.Precision.F32, rgba=rgba, iter=it)
        return rgba, it

    def phoenix(r):
        rgba = np.empty((H2, W2, 4), np.float32)
        it = np.empty((H2, W2), np.int32)
        r.render_phoenix(fr.FractalState(max_iterations=300), W2, H2, precision=fr.Precision.F64, rgba=rgba, iter=it)
        return rgba, it

    fns = {"xD": lambda r: deepx(r, "D"), "xT": lambda r: deepx(r, "T300"), "xB": lambda r: deepx(r, "B"),
           "B": lambda r: deep(r, "B"), "A": lambda r: deep(r, "A"), "dz": deep_zoom, "ph": phoenix}
    alone = {}
    for key, fn in fns.items():
        with fr.Renderer(0) as r:
            alone[key] = fn(r)
    for a, b in zip(alone["xB"], alone["B"]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    with fr.Renderer(0) as r:
        for key in ("xD", "B", "xB", "dz", "xT", "A", "ph", "xD", "xD", "B", "xB", "A", "xT", "dz", "xD"):
            for g, want in zip(fns[key](r), alone[key]):
                assert np.array_equal(np.asarray(g).view(np.uint8), np.asarray(want).view(np.uint8)), key


# 6. what the new entry does not render
def test_unsupported_and_invalid_calls(fr, renderer):
    v = V["D"]
    U, E = fr._capi.FR_ERR_UNSUPPORTED, fr._capi.FR_ERR_INVALID_ARG
    L = fr.lib()
    it = np.empty((8, 8), np.int32)
    o = fr._capi.fr_output(None, None, it.ctypes.data, fr._capi.FR_MEM_HOST, 0)
    cv = fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"]).to_cx()

    def call(view=cv, ftype=fr.FractalType.Mandelbrot, prec=fr.Precision.F64, flags=0, **state):
        p = fr.FractalState(max_iterations=64, **state).to_params(ftype, prec, False)
        p.flags |= flags
        return L.fr_render_deepx(renderer._ctx, C.byref(p), C.byref(view), 8, 8, None, C.byref(o))

    assert call() == 0
    assert call(flags=fr.FR_FLAG_DEEP_BLA) == U
    with pytest.raises(fr.FractalRendererError):
        _render_x(fr, renderer, v, w=8, h=8, bla=True)
    assert call(ftype=fr.FractalType.JuliaSet) == U and call(prec=fr.Precision.F32) == U
    assert call(orbit_trap_enabled=True) == U and call(stripe_enabled=True) == U and call(interior_style=2) == U
    assert call(zoom=0.0) == 0 and call(center_x=float("nan")) == 0            # p->zoom and the double centre are not read
    for bad in (dict(zoom="1e-1001"), dict(zoom="2e3"), dict(zoom="z"), dict(frac_bits=100), dict(center_x="1e")):
        kw = dict(center_x=v["cx"], center_y=v["cy"], zoom=v["zoom"])
        kw.update(bad)
        assert call(view=fr.DeepView(**kw).to_cx()) == E, bad
    bv = fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"]).to_cx()
    bv.reserved = 1
    assert call(view=bv) == E
