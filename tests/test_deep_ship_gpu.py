"""Deep Burning Ship views on the GPU (fr_render_deep_ship): against the fp64 restatement of the folded perturbation step
on every pixel, against the direct fixed-point iteration where fp64 collapses, against fr_render's Burning Ship on shallow
views, shards, layouts, memory kinds, the asynchronous form, and the orbit cache next to fr_render_deep's on one context."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_ref as R
import deep_ship_ref as S

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
    r.render_deep_ship(_state(fr, v, aa), w, h, fr.DeepView(v["cx"], v["cy"]), post_chain=post, rgba=rgba, nu=nu, iter=it,
                       shard=shard)
    return rgba, nu, it


def _render_mandelbrot(fr, r, v, w, h):
    rgba = np.empty((h, w, 4), np.float32)
    nu = np.empty((h, w), np.float64)
    it = np.empty((h, w), np.int32)
    r.render_deep(_state(fr, v), w, h, fr.DeepView(v["cx"], v["cy"]), post_chain=True, rgba=rgba, nu=nu, iter=it)
    return rgba, nu, it


def _same(got, want):
    return all(np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)) for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def _restated(name, aa):
    """computed once per (view, aa), shared, never changed"""
    return S.restate(S.VIEWS[name], W, H, aa)[0]


@functools.lru_cache(maxsize=None)
def _random_pixels():
    rng = np.random.default_rng(99)
    return rng.integers(0, H, 256), rng.integers(0, W, 256)


@functools.lru_cache(maxsize=None)
def _exact(name):
    v = S.VIEWS[name]
    ys, xs = _random_pixels()
    return np.array([S.exact_iter(v["cx"], v["cy"], int(x), int(y), W, H, v["zoom"], v["max_iter"]) for x, y in zip(xs, ys)])


def _expected_rgba(oracle, v, samples, aa, post):
    """the colour stage of the fp64 Burning Ship path on the restated samples: per-sample colour (interior black), the aa
    average in the shader's order, then the post chain with the Burning Ship floors"""
    p = oracle.OracleParams(fractal=2, max_iterations=v["max_iter"], zoom=v["zoom"], aa=aa, post_chain=0)
    acc = np.zeros((H, W, 3), np.float32)
    for it, r2 in samples:
        acc = acc + oracle.colorize(p, S.smooth(it, r2, v["max_iter"]))[..., :3]
    if aa > 1:
        acc = acc / np.float32(aa * aa)
    if post:
        flat = acc.reshape(-1, 3)
        acc = np.array([oracle.post_chain(c, julia_floors=1) for c in flat], np.float32).reshape(H, W, 3)
    return acc


@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("aa", [1, 2])
@pytest.mark.parametrize("name", ["shallow", "A", "B"])
def test_planes_match_the_restatement(fr, renderer, oracle, name, aa, post):
    v = S.VIEWS[name]
    rgba, nu, it = _render(fr, renderer, v, aa, post)
    samples = _restated(name, aa)
    r_it, r_r2 = samples[0]
    print(name, aa, post, "iter mismatches", int((it != r_it).sum()), "escaped", float((r_it < v["max_iter"]).mean()))
    assert np.array_equal(it, r_it), int((it != r_it).sum())
    dnu = np.abs(nu - S.smooth(r_it, r_r2, v["max_iter"])).max()
    print("max |dnu|", dnu)
    assert dnu <= NU_TOL
    assert np.all(rgba[..., 3] == 1.0)
    d = np.abs(rgba[..., :3] - _expected_rgba(oracle, v, samples, aa, post)).max(axis=2)
    bad = d > RGB_TOL
    print("rgb over tolerance", int(bad.sum()), "median", float(np.median(d)))
    assert _few(bad, W * H), int(bad.sum())
    if aa == 1 and not post:
        assert np.all(rgba[..., :3][r_it == v["max_iter"]] == 0.0)                    # interior samples are black


@pytest.mark.parametrize("name", ["A", "B"])
def test_deep_views_are_exact_where_fp64_collapses(fr, renderer, name):
    v = S.VIEWS[name]
    _, _, it = _render(fr, renderer, v)
    ys, xs = _random_pixels()
    ex = _exact(name)
    largest = np.unique(ex, return_counts=True)[1].max() / len(ex)
    agreement = (it[ys, xs] == ex).mean()
    print(name, "largest exact class", largest, "agreement", agreement)
    assert largest <= 0.60                            # a collapsed frame cannot agree by chance
    assert agreement >= 0.99
    # fr_render's Burning Ship in fp64 at the double nearest to the centre: the pixel spacing is far below one ulp of it
    st = fr.FractalState(center_x=float(v["cx"]), center_y=float(v["cy"]), zoom=v["zoom"], max_iterations=v["max_iter"])
    it64 = np.empty((H, W), np.int32)
    renderer.render(st, W, H, fractal_type=fr.FractalType.BurningShip, precision=fr.Precision.F64, iter=it64)
    print("distinct iter values: fr_render", len(np.unique(it64)), "deep", len(np.unique(it)))
    assert len(np.unique(it64)) <= 4
    assert len(np.unique(it)) >= 40


@pytest.mark.parametrize("name", ["shallow", "needle"])
def test_shallow_views_agree_with_fr_render(fr, renderer, name):
    v = S.VIEWS[name]
    _, _, it = _render(fr, renderer, v)
    st = fr.FractalState(center_x=float(v["cx"]), center_y=float(v["cy"]), zoom=v["zoom"], max_iterations=v["max_iter"])
    it64 = np.empty((H, W), np.int32)
    renderer.render(st, W, H, fractal_type=fr.FractalType.BurningShip, precision=fr.Precision.F64, iter=it64)
    print(name, "agreement with fr_render", float((it == it64).mean()))
    assert (it == it64).mean() >= 0.98


def test_shards_layouts_memory_and_async(fr, renderer):
    import torch
    v = S.SHIP_A
    w, h = 203, 117
    ref = _render(fr, renderer, v, 2, True, w=w, h=h)
    ref_rgba, ref_nu, ref_it = ref
    assert renderer.last_kernel_ms() > 0.0 and renderer.last_grid() > 0
    assert _same(_render(fr, renderer, v, 2, True, w=w, h=h), ref)                    # twice: identical bytes
    # host planes, 3 parts of strips
    for strip in (None, 8):
        rgba = np.zeros_like(ref_rgba); nu = np.zeros_like(ref_nu); it = np.full_like(ref_it, -7)
        for part in range(3):
            sh = fr.Shard(part, 3) if strip is None else fr.Shard(part, 3, strip)
            g = sh.global_rows(h)
            a, n, i = _render(fr, renderer, v, 2, True, shard=sh, w=w, h=h)
            rgba[g], nu[g], it[g] = a, n, i
        assert _same((rgba, nu, it), ref), strip
    dev = torch.device("cuda:0")
    st = _state(fr, v, 2)
    view = fr.DeepView(v["cx"], v["cy"])
    # device planes, synchronous and asynchronous on a caller's stream
    for sync in (True, False):
        d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
        d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
        d_it = torch.zeros((h, w), dtype=torch.int32, device=dev)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        if sync:
            renderer.render_deep_ship(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it)
        else:
            renderer.render_deep_ship(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it,
                                      stream=s.cuda_stream, sync=False)
            s.synchronize()
            renderer.check()
        assert _same((d_rgba.cpu().numpy(), d_nu.cpu().numpy(), d_it.cpu().numpy()), ref), sync
    # FR_LAYOUT_FRAME: each part writes its rows in place into whole-frame device planes
    L = fr.lib()
    p = st.to_params(fr.FractalType.BurningShip, fr.Precision.F64, True)
    cv = view.to_c()
    d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
    d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
    d_it = torch.full((h, w), -7, dtype=torch.int32, device=dev)
    o = fr._capi.fr_output(d_rgba.data_ptr(), d_nu.data_ptr(), d_it.data_ptr(), fr._capi.FR_MEM_DEVICE, fr._capi.FR_LAYOUT_FRAME)
    torch.cuda.synchronize()
    for part in range(3):
        sh = fr._capi.fr_shard(part, 3, 16)
        assert L.fr_render_deep_ship(renderer._ctx, C.byref(p), C.byref(cv), w, h, C.byref(sh), C.byref(o)) == 0
    assert _same((d_rgba.cpu().numpy(), d_nu.cpu().numpy(), d_it.cpu().numpy()), ref)
    # the asynchronous form takes device planes only; FR_LAYOUT_FRAME needs them too
    host = fr._capi.fr_output(ref_rgba.ctypes.data, None, None, fr._capi.FR_MEM_HOST, 0)
    assert L.fr_render_deep_ship_async(renderer._ctx, C.byref(p), C.byref(cv), w, h, None, C.byref(host), None) \
        == fr._capi.FR_ERR_INVALID_ARG
    # the options that have no effect on it are accepted
    renderer.set_option("periodicity", 1)
    renderer.set_option("staging", 1)
    got = _render(fr, renderer, v, 2, True, w=w, h=h)
    renderer.set_option("periodicity", 0)
    renderer.set_option("staging", 0)
    assert _same(got, ref)


def test_ship_and_mandelbrot_orbits_do_not_evict_each_other(fr):
    W2, H2 = 160, 120
    with fr.Renderer(0) as r:
        ship_alone = _render(fr, r, S.SHIP_A, 1, True, w=W2, h=H2)
    with fr.Renderer(0) as r:
        mand_alone = _render_mandelbrot(fr, r, R.VIEW_A, W2, H2)
    with fr.Renderer(0) as r:
        assert _same(_render_mandelbrot(fr, r, R.VIEW_A, W2, H2), mand_alone)
        assert _same(_render(fr, r, S.SHIP_A, 1, True, w=W2, h=H2), ship_alone)
        assert _same(_render_mandelbrot(fr, r, R.VIEW_A, W2, H2), mand_alone)
        assert _same(_render(fr, r, S.SHIP_A, 1, True, w=W2, h=H2), ship_alone)
        _render(fr, r, S.SHIP_B, 1, True, w=W2, h=H2)         # another ship view: the ship's slot alone changes
        assert _same(_render_mandelbrot(fr, r, R.VIEW_A, W2, H2), mand_alone)
        assert _same(_render(fr, r, S.SHIP_A, 1, True, w=W2, h=H2), ship_alone)
