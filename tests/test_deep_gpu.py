"""Deep Mandelbrot views on the GPU (fr_render_deep): against the fp64 restatement of the perturbation step on every
pixel, against the direct fixed-point iteration where fp64 collapses, against fr_render on the default view, shards,
layouts, memory kinds, the asynchronous form and the orbit cache next to the other paths on one context."""
import functools

import numpy as np
import pytest

import deep_ref as R

pytestmark = pytest.mark.gpu

W, H = 256, 192
RGB_TOL = 1e-4
NU_TOL = 1e-9


def _few(bad, n):
    """palette wrap exceptions: a sample whose t sits on a knot or on fract's wrap may take the neighbouring colour"""
    return int(bad.sum()) <= max(2, int(0.001 * n))


def _state(fr, v, aa=1):
    return fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"], antialiasing_samples=aa)


def _render(fr, r, v, aa=1, post=False, shard=None, w=W, h=H):
    rows = shard.rows(h) if shard else h
    rgba = np.empty((rows, w, 4), np.float32)
    nu = np.empty((rows, w), np.float64)
    it = np.empty((rows, w), np.int32)
    r.render_deep(_state(fr, v, aa), w, h, fr.DeepView(v["cx"], v["cy"]), post_chain=post, rgba=rgba, nu=nu, iter=it,
                  shard=shard)
    return rgba, nu, it


@functools.lru_cache(maxsize=None)
def _restated(name, aa):
    samples, _ = R.restate(R.VIEWS[name], W, H, aa)
    return samples


def _expected_rgba(oracle, v, samples, aa, post):
    """the colour stage of the fp64 Mandelbrot path on the restated samples: per-sample colour, the aa average in the
    shader's order, then the post chain"""
    p = oracle.OracleParams(max_iterations=v["max_iter"], zoom=v["zoom"], aa=aa, post_chain=0)
    acc = np.zeros((H, W, 3), np.float32)
    for it, r2 in samples:
        acc = acc + oracle.colorize(p, R.smooth(it, r2, v["max_iter"]))[..., :3]
    if aa > 1:
        acc = acc / np.float32(aa * aa)
    if post:
        flat = acc.reshape(-1, 3)
        acc = np.array([oracle.post_chain(c) for c in flat], np.float32).reshape(H, W, 3)
    return acc


@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("aa", [1, 2])
@pytest.mark.parametrize("name", ["shallow", "A", "B"])
def test_planes_match_the_restatement(fr, renderer, oracle, name, aa, post):
    v = R.VIEWS[name]
    rgba, nu, it = _render(fr, renderer, v, aa, post)
    samples = _restated(name, aa)
    r_it, r_r2 = samples[0]
    assert np.array_equal(it, r_it), int((it != r_it).sum())
    assert np.abs(nu - R.smooth(r_it, r_r2, v["max_iter"])).max() <= NU_TOL
    assert np.all(rgba[..., 3] == 1.0)
    bad = np.abs(rgba[..., :3] - _expected_rgba(oracle, v, samples, aa, post)).max(axis=2) > RGB_TOL
    assert _few(bad, W * H), int(bad.sum())


@pytest.mark.parametrize("name", ["A", "B"])
def test_deep_views_are_exact_where_fp64_collapses(fr, renderer, name):
    v = R.VIEWS[name]
    _, _, it = _render(fr, renderer, v)
    rng = np.random.default_rng(99)
    ys, xs = rng.integers(0, H, 256), rng.integers(0, W, 256)
    ex = np.array([R.exact_iter(v["cx"], v["cy"], int(x), int(y), W, H, v["zoom"], v["max_iter"]) for x, y in zip(xs, ys)])
    assert np.unique(ex, return_counts=True)[1].max() <= 0.60 * len(ex)   # a collapsed frame cannot agree by chance
    assert (it[ys, xs] == ex).mean() >= 0.99
    # fr_render in fp64 at the double nearest to the centre: the pixel spacing is far below one ulp of it
    st = fr.FractalState(center_x=float(v["cx"]), center_y=float(v["cy"]), zoom=v["zoom"], max_iterations=v["max_iter"])
    it64 = np.empty((H, W), np.int32)
    renderer.render(st, W, H, precision=fr.Precision.F64, iter=it64)
    assert (it64[ys, xs] != ex).mean() >= 0.20


def test_shallow_view_agrees_with_fr_render(fr, renderer):
    v = R.SHALLOW
    _, _, it = _render(fr, renderer, v)
    it64 = np.empty((H, W), np.int32)
    renderer.render(_state(fr, v), W, H, precision=fr.Precision.F64, iter=it64)
    assert (it == it64).mean() >= 0.99


def test_shards_layouts_memory_and_async(fr, renderer):
    import torch
    v = R.VIEW_A
    w, h = 203, 117
    ref_rgba, ref_nu, ref_it = _render(fr, renderer, v, 2, True, w=w, h=h)
    assert renderer.last_kernel_ms() > 0.0 and renderer.last_grid() > 0
    for nparts in (1, 3, 8):
        rgba = np.zeros_like(ref_rgba); nu = np.zeros_like(ref_nu); it = np.full_like(ref_it, -7)
        for part in range(nparts):
            sh = fr.Shard(part, nparts)
            g = sh.global_rows(h)
            a, n, i = _render(fr, renderer, v, 2, True, shard=sh, w=w, h=h)
            rgba[g], nu[g], it[g] = a, n, i
        assert np.array_equal(rgba, ref_rgba) and np.array_equal(nu.view(np.uint64), ref_nu.view(np.uint64)) \
            and np.array_equal(it, ref_it), nparts
    dev = torch.device("cuda:0")
    st = _state(fr, v, 2)
    view = fr.DeepView(v["cx"], v["cy"])
    # device planes, synchronous and asynchronous on a torch stream
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
    import ctypes as C
    L = fr.lib()
    p = st.to_params(fr.FractalType.Mandelbrot, fr.Precision.F64, True)
    cv = view.to_c()
    d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
    d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
    d_it = torch.full((h, w), -7, dtype=torch.int32, device=dev)
    o = fr._capi.fr_output(d_rgba.data_ptr(), d_nu.data_ptr(), d_it.data_ptr(), fr._capi.FR_MEM_DEVICE, fr._capi.FR_LAYOUT_FRAME)
    torch.cuda.synchronize()
    for part in range(3):
        sh = fr._capi.fr_shard(part, 3, 16)
        assert L.fr_render_deep(renderer._ctx, C.byref(p), C.byref(cv), w, h, C.byref(sh), C.byref(o)) == 0
    assert np.array_equal(d_rgba.cpu().numpy(), ref_rgba) and np.array_equal(d_it.cpu().numpy(), ref_it)
    assert np.array_equal(d_nu.cpu().numpy().view(np.uint64), ref_nu.view(np.uint64))
    # the options that have no effect on it are accepted
    renderer.set_option("periodicity", 1)
    renderer.set_option("staging", 1)
    a, n, i = _render(fr, renderer, v, 2, True, w=w, h=h)
    renderer.set_option("periodicity", 0)
    renderer.set_option("staging", 0)
    assert np.array_equal(a, ref_rgba) and np.array_equal(i, ref_it)


def test_orbit_cache_and_buffers_do_not_leak_between_paths(fr):
    W2, H2 = 160, 120

    def deep(r, name):
        return _render(fr, r, R.VIEWS[name], 1, True, w=W2, h=H2)

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

    alone = {}
    for key, fn in (("A", lambda r: deep(r, "A")), ("B", lambda r: deep(r, "B")), ("dz", deep_zoom), ("ph", phoenix)):
        with fr.Renderer(0) as r:
            alone[key] = fn(r)
    with fr.Renderer(0) as r:
        for key in ("A", "dz", "B", "ph", "A", "A", "dz", "B"):
            got = deep(r, key) if key in ("A", "B") else (deep_zoom(r) if key == "dz" else phoenix(r))
            for g, want in zip(got, alone[key]):
                assert np.array_equal(np.asarray(g).view(np.uint8), np.asarray(want).view(np.uint8)), key
