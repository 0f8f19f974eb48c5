"""Deep Phoenix views on the GPU (fr_render_deep_phoenix): against the fp64 restatement of the second-order perturbation step on
every pixel, against the direct fixed-point iteration where fp64 collapses, against fr_render_phoenix on shallow views, shards,
layouts, memory kinds, the asynchronous form, the orbit cache and its key, and the smallest iteration counts and orbits."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_phoenix_ref as D
import deep_ref as R
import phoenix_ref as PH

pytestmark = pytest.mark.gpu

W, H = 48, 36
SMALL = (24, 18)
RAGGED = (71, 53)                  # no multiple of the 8 x 8 sub-tile either way: the sub-tile tails
RGB_TOL = 1e-4
NU_TOL = 1e-9                      # NU_TOL of test_deep_ship_gpu.py, NU_TOL_F64 of test_phoenix_gpu.py: only log differs
PHOENIX = 3                        # the formula index of the Phoenix slot (fr_deep_orbit_generation)


def _few(bad, n):
    """test_phoenix_gpu.py's cap -- palette wrap exceptions: a sample whose t sits on a knot or on fract's wrap may take the
    neighbouring colour.  (The restatement against itself leaves nothing out: test_deep_phoenix_host.py.)"""
    return int(bad.sum()) <= max(2, int(0.001 * n))


def _state(fr, v, aa=1, density=0.0, **kw):
    return fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"], antialiasing_samples=aa, stripe_density=density, **kw)


def _ph(fr, v):
    return fr.PhoenixParams(phoenix_p=v["p"], phoenix_r=v["r"])


def _render(fr, r, v, aa=1, post=False, density=0.0, shard=None, w=W, h=H):
    rows = shard.rows(h) if shard else h
    rgba = np.empty((rows, w, 4), np.float32)
    nu = np.empty((rows, w), np.float64)
    it = np.empty((rows, w), np.int32)
    r.render_deep_phoenix(_state(fr, v, aa, density), w, h, fr.DeepView(v["cx"], v["cy"]), _ph(fr, v), post_chain=post, rgba=rgba,
                          nu=nu, iter=it, shard=shard)
    return rgba, nu, it


def _same(got, want):
    return all(np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)) for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def _samples(name, w, h, aa):
    """computed once per (view, size, aa), shared, never changed"""
    return D.samples(D.VIEWS[name], w, h, aa)[0]


def _check_planes(name, got, w, h, aa, post, density):
    v = D.VIEWS[name]
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


@pytest.mark.parametrize("density", [0.0, 10.0])
@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("aa", [1, 2])
@pytest.mark.parametrize("name", ["shallowA", "shallowB", "PA30", "PB30", "PA", "PB"])
def test_planes_match_the_restatement(fr, renderer, name, aa, post, density):
    _check_planes(name, _render(fr, renderer, D.VIEWS[name], aa, post, density), W, H, aa, post, density)


@pytest.mark.parametrize("name,size,aa", [("PB30", SMALL, 3), ("PA30", SMALL, 1), ("PA30", RAGGED, 2), ("shallowB", RAGGED, 1),
                                          ("miniR", SMALL, 1), ("mini0", SMALL, 2)])
def test_planes_at_other_sizes_and_aa_3(fr, renderer, name, size, aa):
    w, h = size
    _check_planes(name, _render(fr, renderer, D.VIEWS[name], aa, True, 10.0, w=w, h=h), w, h, aa, True, 10.0)


@pytest.mark.parametrize("name", ["PA30", "PA"])
def test_deep_views_are_exact_where_fp64_collapses(fr, renderer, name):
    v = D.VIEWS[name]
    w, h = SMALL
    _, _, it = _render(fr, renderer, v, w=w, h=h)
    ex = D.exact_frame(v, w, h)
    print(name, "mismatches against the exact iteration", int((it != ex).sum()), "distinct", len(np.unique(ex)))
    assert np.array_equal(it, ex)
    assert len(np.unique(ex)) >= 17 and 0.2 <= (ex == v["max_iter"]).mean() <= 0.8
    # fr_render_phoenix in fp64 at the double nearest to the centre: the pixel spacing is far below one ulp of it
    st = fr.FractalState(center_x=float(v["cx"]), center_y=float(v["cy"]), zoom=v["zoom"], max_iterations=v["max_iter"])
    it64 = np.empty((h, w), np.int32)
    renderer.render_phoenix(st, w, h, _ph(fr, v), precision=fr.Precision.F64, iter=it64)
    print("distinct iter values: fr_render_phoenix", len(np.unique(it64)), "deep", len(np.unique(it)))
    assert len(np.unique(it64)) < 3


@pytest.mark.parametrize("name", ["shallowA", "shallowB"])
def test_shallow_views_agree_with_fr_render_phoenix(fr, renderer, name):
    """iter equal on all but boundary pixels.  The bound is the mismatch count of the restatement against the fp64 restatement of
    fr_render_phoenix on the same frame, taken here: 0 at 48 x 36 for either (p, r) (also 0 at 24 x 18 and 71 x 53)."""
    v = D.VIEWS[name]
    _, _, it = _render(fr, renderer, v)
    st = fr.FractalState(center_x=float(v["cx"]), center_y=float(v["cy"]), zoom=v["zoom"], max_iterations=v["max_iter"])
    it64 = np.empty((H, W), np.int32)
    renderer.render_phoenix(st, W, H, _ph(fr, v), precision=fr.Precision.F64, iter=it64)
    r_it = _samples(name, W, H, 1)[0][0]
    p_it = PH.render(W, H, center_x=float(v["cx"]), center_y=float(v["cy"]), zoom=v["zoom"], max_iterations=v["max_iter"],
                     phoenix_p=v["p"], phoenix_r=v["r"], f64=True)[0]
    bound = int((r_it != p_it).sum())
    print(name, "mismatches: device", int((it != it64).sum()), "restatements", bound)
    assert bound == 0
    assert int((it != it64).sum()) <= bound
    assert len(np.unique(it)) >= 15


def test_shards_layouts_memory_and_async(fr, renderer):
    import torch
    v = D.PA30
    w, h = RAGGED
    ref = _render(fr, renderer, v, 2, True, 10.0, w=w, h=h)
    ref_rgba, ref_nu, ref_it = ref
    assert renderer.last_kernel_ms() > 0.0 and renderer.last_grid() > 0
    assert _same(_render(fr, renderer, v, 2, True, 10.0, w=w, h=h), ref)              # twice: identical bytes
    # host planes, 3 parts of strips
    for strip in (None, 8):
        rgba = np.zeros_like(ref_rgba); nu = np.zeros_like(ref_nu); it = np.full_like(ref_it, -7)
        for part in range(3):
            sh = fr.Shard(part, 3) if strip is None else fr.Shard(part, 3, strip)
            g = sh.global_rows(h)
            a, n, i = _render(fr, renderer, v, 2, True, 10.0, shard=sh, w=w, h=h)
            rgba[g], nu[g], it[g] = a, n, i
        assert _same((rgba, nu, it), ref), strip
    dev = torch.device("cuda:0")
    st = _state(fr, v, 2, 10.0)
    view = fr.DeepView(v["cx"], v["cy"])
    ph = _ph(fr, v)
    # device planes, synchronous and asynchronous on a caller's stream
    for sync in (True, False):
        d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
        d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
        d_it = torch.zeros((h, w), dtype=torch.int32, device=dev)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        if sync:
            renderer.render_deep_phoenix(st, w, h, view, ph, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it)
        else:
            renderer.render_deep_phoenix(st, w, h, view, ph, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it,
                                         stream=s.cuda_stream, sync=False)
            s.synchronize()
            renderer.check()
        assert _same((d_rgba.cpu().numpy(), d_nu.cpu().numpy(), d_it.cpu().numpy()), ref), sync
    # FR_LAYOUT_FRAME: each part writes its rows in place into whole-frame device planes
    L = fr.lib()
    p = st.to_params(fr.FractalType.Phoenix, fr.Precision.F64, True)
    cv = view.to_c()
    cph = ph.to_c()
    d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
    d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
    d_it = torch.full((h, w), -7, dtype=torch.int32, device=dev)
    o = fr._capi.fr_output(d_rgba.data_ptr(), d_nu.data_ptr(), d_it.data_ptr(), fr._capi.FR_MEM_DEVICE, fr._capi.FR_LAYOUT_FRAME)
    torch.cuda.synchronize()
    for part in range(3):
        sh = fr._capi.fr_shard(part, 3, 16)
        assert L.fr_render_deep_phoenix(renderer._ctx, C.byref(p), C.byref(cph), C.byref(cv), w, h, C.byref(sh), C.byref(o)) == 0
    assert _same((d_rgba.cpu().numpy(), d_nu.cpu().numpy(), d_it.cpu().numpy()), ref)
    # the asynchronous form takes device planes only
    host = fr._capi.fr_output(ref_rgba.ctypes.data, None, None, fr._capi.FR_MEM_HOST, 0)
    assert L.fr_render_deep_phoenix_async(renderer._ctx, C.byref(p), C.byref(cph), C.byref(cv), w, h, None, C.byref(host), None) \
        == fr._capi.FR_ERR_INVALID_ARG
    # what Phoenix does not read changes no byte
    got = np.empty_like(ref_rgba), np.empty_like(ref_nu), np.empty_like(ref_it)
    renderer.render_deep_phoenix(_state(fr, v, 2, 10.0, bailout=100.0, color_offset=0.3, interior_style=2, stripe_enabled=True,
                                        center_x=1.5, center_y=-7.0), w, h, view, ph, post_chain=True, rgba=got[0], nu=got[1],
                                 iter=got[2])
    assert _same(got, ref)


def test_orbit_cache_and_its_key(fr):
    """a second render of the view is launch-only (the slot's generation stays); p, r, max_iter, F or the centre recompute"""
    L = fr.lib()
    v = D.PB30
    w, h = SMALL
    with fr.Renderer(0) as r:
        gen = lambda: int(L.fr_deep_orbit_generation(r._ctx, 0, PHOENIX))
        assert gen() == 0
        first = _render(fr, r, v, w=w, h=h)
        assert gen() == 1
        assert _same(_render(fr, r, v, w=w, h=h), first) and gen() == 1
        _render(fr, r, v, 2, True, 10.0, w=w, h=h)                 # aa, colour, post chain and the frame size are not in the key
        _render(fr, r, v, w=W, h=H)
        assert gen() == 1
        for k, other in enumerate([dict(v, p=0.2500001), dict(v, r=-0.3750001), dict(v, max_iter=v["max_iter"] - 1),
                                   dict(v, cx=v["cx"] + "0"), dict(v, p=0.25, r=-0.375)]):
            _render(fr, r, other, w=w, h=h)
            assert gen() == 2 + k, other
        # p->bailout is not read, so it is not in the key either
        it = np.empty((h, w), np.int32)
        r.render_deep_phoenix(_state(fr, v, bailout=7.0), w, h, fr.DeepView(v["cx"], v["cy"]), _ph(fr, v), iter=it)
        assert gen() == 6 and np.array_equal(it, first[2])
        _render(fr, r, dict(v, zoom=2e-30), w=w, h=h)              # the same F (256 bits either way): the zoom is no key
        assert gen() == 6
        for f in (0, 1, 2):                                        # nobody else's slot was touched
            assert int(L.fr_deep_orbit_generation(r._ctx, 0, f)) == 0 and int(L.fr_deep_orbit_generation(r._ctx, 1, f)) == 0


def test_phoenix_and_mandelbrot_orbits_do_not_evict_each_other(fr):
    L = fr.lib()
    w, h = SMALL

    def mandel(r):
        v = R.VIEW_A
        rgba = np.empty((h, w, 4), np.float32); nu = np.empty((h, w), np.float64); it = np.empty((h, w), np.int32)
        r.render_deep(fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"]), w, h, fr.DeepView(v["cx"], v["cy"]),
                      post_chain=True, rgba=rgba, nu=nu, iter=it)
        return rgba, nu, it

    with fr.Renderer(0) as r:
        phoenix_alone = _render(fr, r, D.PA30, 1, True, 10.0, w=w, h=h)
    with fr.Renderer(0) as r:
        mand_alone = mandel(r)
    with fr.Renderer(0) as r:
        gens = lambda: (int(L.fr_deep_orbit_generation(r._ctx, 0, 0)), int(L.fr_deep_orbit_generation(r._ctx, 0, PHOENIX)))
        assert _same(mandel(r), mand_alone) and gens() == (1, 0)
        assert _same(_render(fr, r, D.PA30, 1, True, 10.0, w=w, h=h), phoenix_alone) and gens() == (1, 1)
        assert _same(mandel(r), mand_alone) and gens() == (1, 1)              # a Phoenix render between two fr_render_deep
        assert _same(_render(fr, r, D.PA30, 1, True, 10.0, w=w, h=h), phoenix_alone) and gens() == (1, 1)   # ... and the reverse
        _render(fr, r, D.PB30, w=w, h=h)                                      # another Phoenix view: its slot alone changes
        assert gens() == (1, 2)
        assert _same(mandel(r), mand_alone) and gens() == (1, 2)


@pytest.mark.parametrize("max_iter", [1, 2, 3])
@pytest.mark.parametrize("centre", [("-0.5", "0"), ("3", "0"), ("1.2", "0"), ("0.8", "0.3")])
def test_smallest_iteration_counts_and_orbits(fr, renderer, centre, max_iter):
    """max_iter 1, 2, 3 and reference orbits of 1 to 3 updates: where the Z_{m-1} / Z_{m+2} indexing and the m == N rebase can
    go wrong.  Centre 3: N = 1 (Z_1 = 3 escapes); 1.2: N = 2; 0.8 + 0.3i: N = 3; -0.5: N = max_iter."""
    v = dict(cx=centre[0], cy=centre[1], zoom=3.0, max_iter=max_iter, p=0.0, r=-0.5)
    w, h = SMALL
    orbit = D.view_orbit(v)
    want_n = {"3": 1, "1.2": 2, "0.8": 3}.get(centre[0], max_iter)
    assert len(orbit) - 1 == min(want_n, max_iter)
    smp, _ = D.samples(v, w, h, 2, orbit=orbit)
    rgba, nu, it = _render(fr, renderer, v, 2, False, 10.0, w=w, h=h)
    r_it, _, r_zx, r_zy = smp[0]
    assert np.array_equal(it, r_it)
    assert np.abs(nu - D.smooth(r_it, r_zx, r_zy, max_iter)).max() <= NU_TOL      # (r2 > 4: the smooth count is finite)
    d = np.abs(rgba[..., :3] - D.colour(smp, max_iter, 10.0)).max(axis=2)
    assert _few(~(d <= RGB_TOL), w * h)
    if max_iter == 3 and centre[0] == "-0.5":
        assert len(np.unique(r_it)) == 4                           # every escape index occurs, and interior
