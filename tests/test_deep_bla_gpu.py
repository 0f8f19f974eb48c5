"""Deep views with bilinear approximation on the GPU (fr_render_deep with FR_FLAG_DEEP_BLA): the planes and the step
counts against the numpy restatement (tests/deep_bla_ref.py), the device-built table against numpy's, the direct
fixed-point iteration, the plain path, shards, layouts, memory kinds, the asynchronous form and the caches of one
context."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_bla_ref as BR
import deep_ref as R
from test_deep_gpu import NU_TOL, RGB_TOL, _expected_rgba, _few

pytestmark = pytest.mark.gpu

W, H = 256, 192
VIEWS = dict(R.VIEWS, C=BR.VIEW_C)


def _state(fr, v, aa=1):
    return fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"], antialiasing_samples=aa)


def _render(fr, r, v, aa=1, post=False, shard=None, w=W, h=H, bla=True):
    rows = shard.rows(h) if shard else h
    rgba = np.empty((rows, w, 4), np.float32)
    nu = np.empty((rows, w), np.float64)
    it = np.empty((rows, w), np.int32)
    r.render_deep(_state(fr, v, aa), w, h, fr.DeepView(v["cx"], v["cy"]), post_chain=post, rgba=rgba, nu=nu, iter=it,
                  shard=shard, bla=bla)
    return rgba, nu, it


@functools.lru_cache(maxsize=None)
def _restated(name, aa):
    return BR.restate_bla(VIEWS[name], W, H, aa)


@pytest.mark.parametrize("name,aa,post", [(n, aa, post) for n in ("shallow", "A", "B") for aa in (1, 2) for post in (False, True)]
                         + [("C", 1, False), ("C", 1, True), ("C", 2, True)])
def test_planes_and_counts_match_the_restatement(fr, renderer, oracle, name, aa, post):
    v = VIEWS[name]
    rgba, nu, it = _render(fr, renderer, v, aa, post)
    samples, counts = _restated(name, aa)
    r_it, r_r2 = samples[0]
    assert np.array_equal(it, r_it), int((it != r_it).sum())
    assert np.abs(nu - R.smooth(r_it, r_r2, v["max_iter"])).max() <= NU_TOL
    assert np.all(rgba[..., 3] == 1.0)
    bad = np.abs(rgba[..., :3] - _expected_rgba(oracle, v, samples, aa, post)).max(axis=2) > RGB_TOL
    assert _few(bad, W * H), int(bad.sum())
    # every table radius and every level choice of the kernel, summed: equal, not close
    assert tuple(renderer.last_deep_steps()) == tuple(counts), (renderer.last_deep_steps(), counts)
    if name != "shallow":
        assert counts[1] > 0


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_device_table_equals_numpy_bit_for_bit(fr, renderer, name):
    """every (A, B, r) the device built, through its sqrt included, against bla_table"""
    v = VIEWS[name]
    _render(fr, renderer, v)
    orb = R.reference_orbit(v["cx"], v["cy"], v["zoom"], v["max_iter"])
    tab = BR.bla_table(orb, BR.dcmax(W, H, v["zoom"]))
    n = sum(len(T["r"]) for T in tab)
    r = np.empty(n, np.float64)
    ab = np.empty((n, 4), np.float64)
    got = fr.lib().fr_deep_bla_table(renderer._ctx, r.ctypes.data, ab.ctypes.data, n)
    assert got == n
    want_r = np.concatenate([T["r"] for T in tab])
    want_ab = np.concatenate([np.stack([T["ax"], T["ay"], T["bx"], T["by"]], axis=1) for T in tab])
    assert np.array_equal(r.view(np.uint64), want_r.view(np.uint64))
    assert np.array_equal(ab.view(np.uint64), want_ab.view(np.uint64))


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_bla_is_exact_where_fp64_collapses(fr, renderer, name):
    v = VIEWS[name]
    _, _, it = _render(fr, renderer, v)
    rng = np.random.default_rng(99)
    ys, xs = rng.integers(0, H, 256), rng.integers(0, W, 256)
    ex = np.array([R.exact_iter(v["cx"], v["cy"], int(x), int(y), W, H, v["zoom"], v["max_iter"]) for x, y in zip(xs, ys)])
    assert (it[ys, xs] == ex).mean() >= 0.99


@pytest.mark.parametrize("name", ["shallow", "A", "B", "C"])
def test_agreement_with_the_plain_path(fr, renderer, name):
    """Share of pixels whose iter equals the plain path's on the same context.  The restatements give 1.0 on the shallow
    view (no BLA step), A and B, and 0.99998 on C (1 pixel of 49152 at 256 x 192: a sample near the minibrot's boundary
    whose escape falls inside a skipped stretch or a rounding away).  The bar, 0.9995, is 25 such pixels."""
    v = VIEWS[name]
    _, _, it_bla = _render(fr, renderer, v)
    _, _, it_plain = _render(fr, renderer, v, bla=False)
    assert (it_bla == it_plain).mean() >= 0.9995


def test_centre_zero_takes_no_bla_step(fr, renderer):
    v = dict(cx="0", cy="0", zoom=1e-20, max_iter=500)
    a, n, i = _render(fr, renderer, v, 2, True)
    assert tuple(renderer.last_deep_steps())[1:] == (0, 0)
    a0, n0, i0 = _render(fr, renderer, v, 2, True, bla=False)
    assert np.array_equal(a.view(np.uint8), a0.view(np.uint8)) and np.array_equal(n.view(np.uint8), n0.view(np.uint8)) \
        and np.array_equal(i, i0)


def test_shards_layouts_memory_and_async(fr, renderer):
    import torch
    v = R.VIEW_B
    w, h = 203, 117
    ref_rgba, ref_nu, ref_it = _render(fr, renderer, v, 2, True, w=w, h=h)
    ref_steps = renderer.last_deep_steps()
    assert ref_steps.bla > 0
    for nparts in (1, 3, 8):
        rgba = np.zeros_like(ref_rgba); nu = np.zeros_like(ref_nu); it = np.full_like(ref_it, -7)
        tot = np.zeros(3, np.int64)
        for part in range(nparts):
            sh = fr.Shard(part, nparts)
            g = sh.global_rows(h)
            a, n, i = _render(fr, renderer, v, 2, True, shard=sh, w=w, h=h)
            rgba[g], nu[g], it[g] = a, n, i
            if sh.rows(h):
                tot += np.array(renderer.last_deep_steps())
        assert np.array_equal(rgba, ref_rgba) and np.array_equal(nu.view(np.uint64), ref_nu.view(np.uint64)) \
            and np.array_equal(it, ref_it), nparts
        assert tuple(tot) == tuple(ref_steps), nparts                   # the counts of a call cover its own pixels
    dev = torch.device("cuda:0")
    st = _state(fr, v, 2)
    view = fr.DeepView(v["cx"], v["cy"])
    for sync in (True, False):
        d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
        d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
        d_it = torch.zeros((h, w), dtype=torch.int32, device=dev)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        if sync:
            renderer.render_deep(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it, bla=True)
        else:
            renderer.render_deep(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it,
                                 stream=s.cuda_stream, sync=False, bla=True)
            s.synchronize()
            renderer.check()
        assert renderer.last_deep_steps() == ref_steps, sync
        assert np.array_equal(d_rgba.cpu().numpy(), ref_rgba) and np.array_equal(d_it.cpu().numpy(), ref_it)
        assert np.array_equal(d_nu.cpu().numpy().view(np.uint64), ref_nu.view(np.uint64)), sync
    # FR_LAYOUT_FRAME: each part writes its rows in place into whole-frame device planes
    L = fr.lib()
    p = st.to_params(fr.FractalType.Mandelbrot, fr.Precision.F64, True)
    p.flags |= fr.FR_FLAG_DEEP_BLA
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


def test_counts_need_a_bla_render(fr):
    with fr.Renderer(0) as r:
        with pytest.raises(fr.FractalRendererError):
            r.last_deep_steps()
        _render(fr, r, R.VIEW_A, w=64, h=48, bla=False)
        with pytest.raises(fr.FractalRendererError):
            r.last_deep_steps()
        _render(fr, r, R.VIEW_A, w=64, h=48)
        assert r.last_deep_steps().plain > 0


def test_caches_across_paths(fr):
    """BLA and plain renders of one view, a zoom change at a fixed centre (the table is rebuilt, the orbit kept),
    another view and a Deep_Zoom render on one context: every frame equals the same frame rendered alone"""
    W2, H2 = 160, 120
    vb2 = dict(R.VIEW_B, zoom=2e-100)

    def deep(r, v, bla):
        out = _render(fr, r, v, 1, True, w=W2, h=H2, bla=bla)
        return out + ((tuple(r.last_deep_steps()),) if bla else ())

    def deep_zoom(r):
        st = fr.FractalState(center_x=-0.743643887037151, center_y=0.131825904205330, zoom=1e-5, max_iterations=512,
                             use_perturbation=True)
        rgba = np.empty((H2, W2, 4), np.float32)
        it = np.empty((H2, W2), np.int32)
        r.render(st, W2, H2, fractal_type=fr.FractalType.Deep_Zoom, precision=fr.Precision.F32, rgba=rgba, iter=it)
        return rgba, it

    jobs = {"Bb": lambda r: deep(r, R.VIEW_B, True), "Bp": lambda r: deep(r, R.VIEW_B, False),
            "B2b": lambda r: deep(r, vb2, True), "Cb": lambda r: deep(r, BR.VIEW_C, True),
            "Ab": lambda r: deep(r, R.VIEW_A, True), "dz": deep_zoom}
    alone = {}
    for key, fn in jobs.items():
        with fr.Renderer(0) as r:
            alone[key] = fn(r)
    with fr.Renderer(0) as r:
        for key in ("Bb", "Bp", "Bb", "B2b", "Bb", "dz", "Cb", "Bp", "Ab", "B2b", "dz", "Bb"):
            got = jobs[key](r)
            for g, want in zip(got, alone[key]):
                assert np.array_equal(np.asarray(g).view(np.uint8), np.asarray(want).view(np.uint8)), key
