"""Deep Phoenix views below 1e-290 on the GPU (fr_render_deepx_phoenix): against the two-mode restatement of the kernel's step on
every pixel, against the direct fixed-point iteration, byte for byte against fr_render_deep_phoenix where both accept the view,
the orbit cache and its key, shards, the asynchronous form, NULL planes, and the smallest iteration counts."""
import functools

import numpy as np
import pytest

import deep_phoenix_ref as D
import deep_ref as R
import deepx_phoenix_ref as PX
from test_deep_phoenix_gpu import NU_TOL, RGB_TOL, _few

pytestmark = pytest.mark.gpu

W, H = 48, 36
SMALL = PX.GOLDEN_SIZE             # 24 x 18
RAGGED = (71, 53)                  # no multiple of the 8 x 8 sub-tile either way: the sub-tile tails
PHOENIX = 3                        # the formula index of the Phoenix slots (fr_deep_orbit_generation)
VIEWS = {**PX.NEW_VIEWS, **PX.OLD_VIEWS}


def _state(fr, v, aa=1, density=0.0, **kw):
    return fr.FractalState(max_iterations=v["max_iter"], antialiasing_samples=aa, stripe_density=density, **kw)


def _ph(fr, v):
    return fr.PhoenixParams(phoenix_p=v["p"], phoenix_r=v["r"])


def _dv(fr, v):
    return fr.DeepView(v["cx"], v["cy"], v.get("frac_bits", 0), zoom=v["zoom"])


def _render(fr, r, v, aa=1, post=False, density=0.0, shard=None, w=W, h=H):
    rows = shard.rows(h) if shard else h
    rgba = np.empty((rows, w, 4), np.float32)
    nu = np.empty((rows, w), np.float64)
    it = np.empty((rows, w), np.int32)
    r.render_deepx_phoenix(_state(fr, v, aa, density), w, h, _dv(fr, v), _ph(fr, v), post_chain=post, rgba=rgba, nu=nu, iter=it,
                           shard=shard)
    return rgba, nu, it


def _same(got, want):
    return all(np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)) for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def _samples(name, w, h, aa):
    """computed once per (view, size, aa), shared, never changed"""
    return PX.samples_x(VIEWS[name], w, h, aa)


def _check_planes(name, got, w, h, aa, post, density):
    v = VIEWS[name]
    rgba, nu, it = got
    smp = _samples(name, w, h, aa)
    r_it, _, r_zx, r_zy = smp[0]
    print(name, (w, h), aa, post, density, "iter mismatches", int((it != r_it).sum()), "escaped", float((r_it < v["max_iter"]).mean()))
    assert np.array_equal(it, r_it), int((it != r_it).sum())
    dnu = np.abs(nu - D.smooth(r_it, r_zx, r_zy, v["max_iter"])).max()
    print("max |dnu|", dnu)
    assert dnu <= NU_TOL
    assert np.all(rgba[..., 3] == 1.0)
    d = np.abs(rgba[..., :3] - D.colour(smp, v["max_iter"], density, post)).max(axis=2)
    bad = d > RGB_TOL
    print("rgb over tolerance", int(bad.sum()), "median", float(np.median(d)))
    assert _few(bad, w * h), int(bad.sum())


@pytest.mark.parametrize("name", list(PX.NEW_VIEWS))
def test_planes_match_the_restatement(fr, renderer, name):
    _check_planes(name, _render(fr, renderer, VIEWS[name]), W, H, 1, False, 0.0)


@pytest.mark.parametrize("name", ["PX310", "PX400B"])
def test_planes_with_aa_2_the_post_chain_and_stripes(fr, renderer, name):
    _check_planes(name, _render(fr, renderer, VIEWS[name], 2, True, 10.0), W, H, 2, True, 10.0)


def test_planes_on_a_ragged_frame_with_aa_3(fr, renderer):
    w, h = RAGGED
    _check_planes("PX400A", _render(fr, renderer, VIEWS["PX400A"], 3, True, 10.0, w=w, h=h), w, h, 3, True, 10.0)


@pytest.mark.parametrize("name", ["PX310", "PX400A", "TIP1000", "PXRET"])
def test_iter_is_the_exact_iteration(fr, renderer, name):
    w, h = SMALL
    _, _, it = _render(fr, renderer, VIEWS[name], w=w, h=h)
    ex = PX.exact_golden()[name]
    print(name, "mismatches against the exact iteration", int((it != ex).sum()), "distinct", len(np.unique(ex)))
    assert np.array_equal(it, ex)


@pytest.mark.parametrize("aa", [1, 2])
@pytest.mark.parametrize("name", ["PA30", "PB30", "PA", "PB", "shallowA"])
def test_bytes_of_fr_render_deep_phoenix_where_both_accept_the_view(fr, renderer, name, aa):
    v = D.VIEWS[name]
    got = _render(fr, renderer, VIEWS[name], aa, True, 10.0)
    rgba = np.empty((H, W, 4), np.float32)
    nu = np.empty((H, W), np.float64)
    it = np.empty((H, W), np.int32)
    st = fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"], antialiasing_samples=aa, stripe_density=10.0)
    renderer.render_deep_phoenix(st, W, H, fr.DeepView(v["cx"], v["cy"]), _ph(fr, v), post_chain=True, rgba=rgba, nu=nu, iter=it)
    for plane, g, w in zip(("rgba", "nu", "iter"), got, (rgba, nu, it)):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (plane, int((g != w).sum()))
    assert len(np.unique(it)) >= 15


def test_orbit_cache_and_its_key(fr):
    """a second render of the view uploads nothing (the slot's generation stays); p, r, max_iter or the zoom string's F refill"""
    L = fr.lib()
    v = dict(PX.OLD_VIEWS["PB30"])
    w, h = SMALL
    with fr.Renderer(0) as r:
        gen = lambda: int(L.fr_deep_orbit_generation(r._ctx, 1, PHOENIX))
        assert gen() == 0
        first = _render(fr, r, v, w=w, h=h)
        assert gen() == 1
        assert _same(_render(fr, r, v, w=w, h=h), first) and gen() == 1
        _render(fr, r, v, 2, True, 10.0, w=w, h=h)                 # aa, colour, post chain and the frame size are not in the key
        _render(fr, r, v, w=W, h=H)
        assert gen() == 1
        _render(fr, r, dict(v, zoom="2e-30"), w=w, h=h)            # the same F (256 bits either way): the zoom is no key
        assert gen() == 1
        for k, other in enumerate([dict(v, p=0.2500001), dict(v, r=-0.3750001), dict(v, max_iter=v["max_iter"] - 1),
                                   dict(v, zoom="1e-60"), dict(v, frac_bits=512), dict(v, cx=v["cx"] + "0")]):
            _render(fr, r, other, w=w, h=h)
            assert gen() == 2 + k, other
        for f in (0, 1, 2):                                        # nobody else's slot was touched, the fp64 Phoenix slot included
            assert int(L.fr_deep_orbit_generation(r._ctx, 0, f)) == 0 and int(L.fr_deep_orbit_generation(r._ctx, 1, f)) == 0
        assert int(L.fr_deep_orbit_generation(r._ctx, 0, PHOENIX)) == 0


def test_the_two_phoenix_slots_and_fr_render_deepx_do_not_evict_each_other(fr):
    L = fr.lib()
    w, h = SMALL
    vx = PX.PX310
    v64 = D.PA30

    def mandelx(r):
        v = R.VIEW_A
        rgba = np.empty((h, w, 4), np.float32); nu = np.empty((h, w), np.float64); it = np.empty((h, w), np.int32)
        # a view with a zoom string: fr_render_deepx
        r.render_deep(fr.FractalState(max_iterations=v["max_iter"]), w, h, fr.DeepView(v["cx"], v["cy"], zoom=repr(float(v["zoom"]))),
                      rgba=rgba, nu=nu, iter=it)
        return rgba, nu, it

    def phoenix64(r):
        rgba = np.empty((h, w, 4), np.float32); nu = np.empty((h, w), np.float64); it = np.empty((h, w), np.int32)
        r.render_deep_phoenix(fr.FractalState(zoom=v64["zoom"], max_iterations=v64["max_iter"]), w, h,
                              fr.DeepView(v64["cx"], v64["cy"]), _ph(fr, v64), rgba=rgba, nu=nu, iter=it)
        return rgba, nu, it

    with fr.Renderer(0) as r:
        x_alone = _render(fr, r, vx, w=w, h=h)
    with fr.Renderer(0) as r:
        m_alone = mandelx(r)
    with fr.Renderer(0) as r:
        p_alone = phoenix64(r)
    with fr.Renderer(0) as r:
        gens = lambda: (int(L.fr_deep_orbit_generation(r._ctx, 1, PHOENIX)), int(L.fr_deep_orbit_generation(r._ctx, 0, PHOENIX)),
                        int(L.fr_deep_orbit_generation(r._ctx, 1, 0)))
        assert _same(_render(fr, r, vx, w=w, h=h), x_alone) and gens() == (1, 0, 0)
        assert _same(phoenix64(r), p_alone) and gens() == (1, 1, 0)
        assert _same(mandelx(r), m_alone) and gens() == (1, 1, 1)
        assert _same(_render(fr, r, vx, w=w, h=h), x_alone) and gens() == (1, 1, 1)    # behind the two others: nothing uploaded
        assert _same(phoenix64(r), p_alone) and _same(mandelx(r), m_alone) and gens() == (1, 1, 1)
        _render(fr, r, PX.OLD_VIEWS["PB30"], w=w, h=h)                                   # another extended Phoenix view: its slot alone
        assert gens() == (2, 1, 1)
        assert _same(phoenix64(r), p_alone) and _same(mandelx(r), m_alone) and gens() == (2, 1, 1)


def test_shards_async_and_null_planes(fr, renderer):
    import torch
    v = PX.PX310
    w, h = SMALL[0] + 7, SMALL[1] + 5                              # 31 x 23: ragged, small
    ref = _render(fr, renderer, v, 2, True, 10.0, w=w, h=h)
    ref_rgba, ref_nu, ref_it = ref
    assert renderer.last_kernel_ms() > 0.0 and renderer.last_grid() > 0
    # host planes, 3 parts of row strips
    for strip in (None, 4):
        rgba = np.zeros_like(ref_rgba); nu = np.zeros_like(ref_nu); it = np.full_like(ref_it, -7)
        for part in range(3):
            sh = fr.Shard(part, 3) if strip is None else fr.Shard(part, 3, strip)
            g = sh.global_rows(h)
            a, n, i = _render(fr, renderer, v, 2, True, 10.0, shard=sh, w=w, h=h)
            rgba[g], nu[g], it[g] = a, n, i
        assert _same((rgba, nu, it), ref), strip
    # device planes, synchronous and asynchronous on a caller's stream
    dev = torch.device("cuda:0")
    st = _state(fr, v, 2, 10.0)
    for sync in (True, False):
        d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
        d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
        d_it = torch.zeros((h, w), dtype=torch.int32, device=dev)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        if sync:
            renderer.render_deepx_phoenix(st, w, h, _dv(fr, v), _ph(fr, v), post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it)
        else:
            renderer.render_deepx_phoenix(st, w, h, _dv(fr, v), _ph(fr, v), post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it,
                                          stream=s.cuda_stream, sync=False)
            s.synchronize()
            renderer.check()
        assert _same((d_rgba.cpu().numpy(), d_nu.cpu().numpy(), d_it.cpu().numpy()), ref), sync
    # NULL planes one at a time: the two others keep their bytes
    for skip in range(3):
        planes = [np.empty_like(ref_rgba), np.empty_like(ref_nu), np.empty_like(ref_it)]
        kw = {k: p for j, (k, p) in enumerate(zip(("rgba", "nu", "iter"), planes)) if j != skip}
        renderer.render_deepx_phoenix(st, w, h, _dv(fr, v), _ph(fr, v), post_chain=True, **kw)
        assert _same([p for j, p in enumerate(planes) if j != skip], [p for j, p in enumerate(ref) if j != skip]), skip
    # what the entry point does not read changes no byte: state.zoom, the double centre, the bailout
    got = np.empty_like(ref_rgba), np.empty_like(ref_nu), np.empty_like(ref_it)
    renderer.render_deepx_phoenix(_state(fr, v, 2, 10.0, zoom=1e-7, bailout=100.0, center_x=1.5, center_y=-7.0), w, h, _dv(fr, v),
                                  _ph(fr, v), post_chain=True, rgba=got[0], nu=got[1], iter=got[2])
    assert _same(got, ref)


@pytest.mark.parametrize("max_iter", [1, 2, 3])
def test_smallest_iteration_counts(fr, renderer, max_iter):
    """max_iter 1, 2, 3 on TIP1000's centre at zoom 1e-400: the Z_{m+2} index clamp, the m == N rebase and lastZ of a lane that
    is still extended when the loop ends"""
    v = dict(PX.TIP1000, zoom="1e-400", max_iter=max_iter)
    w, h = SMALL
    smp = PX.samples_x(v, w, h, 2)
    rgba, nu, it = _render(fr, renderer, v, 2, False, 10.0, w=w, h=h)
    r_it, _, r_zx, r_zy = smp[0]
    assert np.array_equal(it, r_it)
    assert np.abs(nu - D.smooth(r_it, r_zx, r_zy, max_iter)).max() <= NU_TOL
    d = np.abs(rgba[..., :3] - D.colour(smp, max_iter, 10.0)).max(axis=2)
    assert _few(~(d <= RGB_TOL), w * h)
