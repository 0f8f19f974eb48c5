"""Deep Julia views on the GPU (fr_render_deep_julia): against the fp64 restatement of the two-orbit perturbation step on
every pixel, against the direct fixed-point iteration where fr_render's fp64 Julia collapses, against fr_render on shallow
views, shards, layouts, memory kinds, the asynchronous form, and the orbit cache: keyed by c, next to the other deep paths'."""
import ctypes as C

import numpy as np
import pytest

import deep_julia_ref as J
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
    return fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"], antialiasing_samples=aa, julia_c_real=v["c"][0],
                           julia_c_imag=v["c"][1])


def _render(fr, r, v, aa=1, post=False, shard=None, w=W, h=H):
    rows = shard.rows(h) if shard else h
    rgba = np.empty((rows, w, 4), np.float32)
    nu = np.empty((rows, w), np.float64)
    it = np.empty((rows, w), np.int32)
    r.render_deep_julia(_state(fr, v, aa), w, h, fr.DeepView(v["cx"], v["cy"]), post_chain=post, rgba=rgba, nu=nu, iter=it,
                        shard=shard)
    return rgba, nu, it


def _same(got, want):
    return all(np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)) for g, w in zip(got, want))


def _view(name):
    return J.SHALLOW[int(name)] if name.isdigit() else J.view(name)


def _expected_rgba(oracle, v, samples, aa, post):
    """the colour stage of the fp64 Julia path on the restated samples: per-sample colour (interior black), the aa average
    in the shader's order, then the post chain with the Julia floors"""
    p = oracle.OracleParams(fractal=1, max_iterations=v["max_iter"], zoom=v["zoom"], aa=aa, post_chain=0)
    acc = np.zeros((H, W, 3), np.float32)
    for it, r2 in samples:
        acc = acc + oracle.colorize(p, J.smooth(it, r2, v["max_iter"]))[..., :3]
    if aa > 1:
        acc = acc / np.float32(aa * aa)
    if post:
        flat = acc.reshape(-1, 3)
        acc = np.array([oracle.post_chain(c, julia_floors=1) for c in flat], np.float32).reshape(H, W, 3)
    return acc


@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("aa", [1, 2])
@pytest.mark.parametrize("name", ["RABBIT30", "DENDRITE100", "DUST30", "3"])
def test_planes_match_the_restatement(fr, renderer, oracle, name, aa, post):
    v = _view(name)
    rgba, nu, it = _render(fr, renderer, v, aa, post)
    samples = J.restated(name, aa)[0]
    r_it, r_r2 = samples[0]
    print(name, aa, post, "iter mismatches", int((it != r_it).sum()), "escaped", float((r_it < v["max_iter"]).mean()))
    assert np.array_equal(it, r_it), int((it != r_it).sum())
    dnu = np.abs(nu - J.smooth(r_it, r_r2, v["max_iter"])).max()
    print("max |dnu|", dnu)
    assert dnu <= NU_TOL
    assert np.all(rgba[..., 3] == 1.0)
    d = np.abs(rgba[..., :3] - _expected_rgba(oracle, v, samples, aa, post)).max(axis=2)
    bad = d > RGB_TOL
    print("rgb over tolerance", int(bad.sum()), "median", float(np.median(d)))
    assert _few(bad, W * H), int(bad.sum())
    if aa == 1 and not post:
        assert np.all(rgba[..., :3][r_it == v["max_iter"]] == 0.0)                    # interior samples are black


@pytest.mark.parametrize("name", ["RABBIT30", "DENDRITE100", "DUST30"])
def test_deep_views_are_exact_where_fp64_collapses(fr, renderer, name):
    v = J.view(name)
    _, _, it = _render(fr, renderer, v)
    ys, xs = J.random_pixels(W, H)
    ex = J.exact_samples(name)
    largest = np.unique(ex, return_counts=True)[1].max() / len(ex)
    agreement = (it[ys, xs] == ex).mean()
    print(name, "largest exact class", largest, "agreement", agreement)
    assert largest <= 0.80                            # a collapsed frame cannot agree by chance
    assert agreement >= 0.99
    # fr_render's Julia in fp64 at the double nearest to the centre: the pixel spacing is far below one ulp of it
    st = fr.FractalState(center_x=float(v["cx"]), center_y=float(v["cy"]), zoom=v["zoom"], max_iterations=v["max_iter"],
                         julia_c_real=v["c"][0], julia_c_imag=v["c"][1])
    it64 = np.empty((H, W), np.int32)
    renderer.render(st, W, H, fractal_type=fr.FractalType.JuliaSet, precision=fr.Precision.F64, iter=it64)
    print("distinct iter values: fr_render", len(np.unique(it64)), "deep", len(np.unique(it)))
    assert len(np.unique(it64)) <= 4
    assert len(np.unique(it)) >= 30


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_shallow_views_agree_with_fr_render(fr, renderer, k):
    v = J.SHALLOW[k]
    _, _, it = _render(fr, renderer, v)
    st = fr.FractalState(center_x=float(v["cx"]), center_y=float(v["cy"]), zoom=v["zoom"], max_iterations=v["max_iter"],
                         julia_c_real=v["c"][0], julia_c_imag=v["c"][1])
    it64 = np.empty((H, W), np.int32)
    renderer.render(st, W, H, fractal_type=fr.FractalType.JuliaSet, precision=fr.Precision.F64, iter=it64)
    print(v["name"], "agreement with fr_render", float((it == it64).mean()))
    assert (it == it64).mean() >= 0.98


def test_shards_layouts_memory_and_async(fr, renderer):
    import torch
    v = J.view("RABBIT30")
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
            renderer.render_deep_julia(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it)
        else:
            renderer.render_deep_julia(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it,
                                       stream=s.cuda_stream, sync=False)
            s.synchronize()
            renderer.check()
        assert _same((d_rgba.cpu().numpy(), d_nu.cpu().numpy(), d_it.cpu().numpy()), ref), sync
    # FR_LAYOUT_FRAME: each part writes its rows in place into whole-frame device planes
    L = fr.lib()
    p = st.to_params(fr.FractalType.JuliaSet, fr.Precision.F64, True)
    cv = view.to_c()
    d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
    d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
    d_it = torch.full((h, w), -7, dtype=torch.int32, device=dev)
    o = fr._capi.fr_output(d_rgba.data_ptr(), d_nu.data_ptr(), d_it.data_ptr(), fr._capi.FR_MEM_DEVICE, fr._capi.FR_LAYOUT_FRAME)
    torch.cuda.synchronize()
    for part in range(3):
        sh = fr._capi.fr_shard(part, 3, 16)
        assert L.fr_render_deep_julia(renderer._ctx, C.byref(p), C.byref(cv), w, h, C.byref(sh), C.byref(o)) == 0
    assert _same((d_rgba.cpu().numpy(), d_nu.cpu().numpy(), d_it.cpu().numpy()), ref)
    # the asynchronous form takes device planes only; FR_LAYOUT_FRAME needs them too
    host = fr._capi.fr_output(ref_rgba.ctypes.data, None, None, fr._capi.FR_MEM_HOST, 0)
    assert L.fr_render_deep_julia_async(renderer._ctx, C.byref(p), C.byref(cv), w, h, None, C.byref(host), None) \
        == fr._capi.FR_ERR_INVALID_ARG
    # the options that have no effect on it are accepted
    renderer.set_option("periodicity", 1)
    renderer.set_option("staging", 1)
    got = _render(fr, renderer, v, 2, True, w=w, h=h)
    renderer.set_option("periodicity", 0)
    renderer.set_option("staging", 0)
    assert _same(got, ref)


def test_a_second_c_at_the_same_centre_recomputes_the_orbits(fr):
    """the slot is keyed by the bits of c: same centre strings, F, max_iterations and bailout, another c"""
    w, h = 160, 120
    a = dict(J.SHALLOW[3])
    b = dict(a, c=(-0.12, 0.75))
    with fr.Renderer(0) as r:
        a_alone = _render(fr, r, a, w=w, h=h)
    with fr.Renderer(0) as r:
        b_alone = _render(fr, r, b, w=w, h=h)
    assert not np.array_equal(a_alone[2], b_alone[2])
    b_want = J.restate(b, w, h)[0][0]
    assert np.array_equal(b_alone[2], b_want)
    with fr.Renderer(0) as r:
        assert _same(_render(fr, r, a, w=w, h=h), a_alone)
        assert _same(_render(fr, r, b, w=w, h=h), b_alone)
        assert _same(_render(fr, r, a, w=w, h=h), a_alone)


def test_julia_slots_and_the_other_deep_slots_do_not_evict_each_other(fr):
    W2, H2 = 160, 120
    jv = J.view("DENDRITE30")

    def mandel(r):
        v = R.VIEW_A
        out = np.empty((H2, W2), np.int32)
        r.render_deep(fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"]), W2, H2, fr.DeepView(v["cx"], v["cy"]), iter=out)
        return out

    def ship(r):
        v = S.SHIP_A
        out = np.empty((H2, W2), np.int32)
        r.render_deep_ship(fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"]), W2, H2, fr.DeepView(v["cx"], v["cy"]),
                           iter=out)
        return out

    def julia(r, v=jv):
        return _render(fr, r, v, w=W2, h=H2)[2]

    def juliax(r):
        out = np.empty((H2, W2), np.int32)
        r.render_deep_julia(_state(fr, jv), W2, H2, fr.DeepView(jv["cx"], jv["cy"], zoom=jv["zoom_s"]), iter=out)
        return out

    with fr.Renderer(0) as r:
        m0 = mandel(r)
    with fr.Renderer(0) as r:
        s0 = ship(r)
    with fr.Renderer(0) as r:
        j0 = julia(r)
    assert np.array_equal(j0, J.restate(jv, W2, H2)[0][0])
    with fr.Renderer(0) as r:
        for _ in range(2):
            assert np.array_equal(mandel(r), m0) and np.array_equal(julia(r), j0) and np.array_equal(ship(r), s0)
            assert np.array_equal(juliax(r), j0)
        julia(r, J.view("BASILICA30"))                             # another Julia view: the Julia slot alone changes
        assert np.array_equal(mandel(r), m0) and np.array_equal(ship(r), s0) and np.array_equal(juliax(r), j0)
        assert np.array_equal(julia(r), j0)
