"""Deep Phoenix views below 1e-290 with bilinear approximation on the GPU (fr_render_deepx_phoenix with FR_FLAG_DEEPX_PHOENIX_BLA): the
planes and the step counts against the numpy restatement (tests/deepx_phoenix_bla_ref.py), the device-built table against numpy's
bit for bit, the unflagged path, fr_render_deep_phoenix on the views both accept, short budgets, shards, layouts, memory kinds, the
asynchronous form, the caches of one context and the other paths' counters."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_phoenix_ref as D
import deepx_phoenix_bla_ref as XB
import deepx_phoenix_ref as PX
from test_deep_phoenix_gpu import NU_TOL, RGB_TOL, _few
from test_deepx_phoenix_gpu import PHOENIX, RAGGED, SMALL, _dv, _ph, _same, _state

pytestmark = pytest.mark.gpu

W, H = 48, 36
VIEWS = {**XB.VIEWS, **PX.OLD_VIEWS}
OLD = ("PA30", "PA", "shallowA")


def _render(fr, r, v, aa=1, post=False, density=0.0, shard=None, w=W, h=H, xbla=True):
    rows = shard.rows(h) if shard else h
    rgba = np.empty((rows, w, 4), np.float32)
    nu = np.empty((rows, w), np.float64)
    it = np.empty((rows, w), np.int32)
    r.render_deepx_phoenix(_state(fr, v, aa, density), w, h, _dv(fr, v), _ph(fr, v), post_chain=post, rgba=rgba, nu=nu, iter=it,
                           shard=shard, xbla=xbla)
    return rgba, nu, it


@functools.lru_cache(maxsize=None)
def _orbit(name):
    return PX.orbit_of(VIEWS[name])


@functools.lru_cache(maxsize=None)
def _restated(name, w, h, aa):
    """computed once per (view, size, aa), shared, never changed"""
    return XB.samples_x_bla(VIEWS[name], w, h, aa, orbit=_orbit(name))


def _check_planes(v, got, smp, post, density=0.0):
    rgba, nu, it = got
    r_it, _, r_zx, r_zy = smp[0]
    print("iter mismatches", int((it != r_it).sum()), "of", it.size)
    assert np.array_equal(it, r_it), int((it != r_it).sum())
    dnu = np.abs(nu - D.smooth(r_it, r_zx, r_zy, v["max_iter"])).max()
    print("max |dnu|", dnu)
    assert dnu <= NU_TOL
    assert np.all(rgba[..., 3] == 1.0)
    d = np.abs(rgba[..., :3] - D.colour(smp, v["max_iter"], density, post)).max(axis=2)
    bad = ~(d <= RGB_TOL)
    print("rgb over tolerance", int(bad.sum()))
    assert _few(bad, it.size), int(bad.sum())


@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("aa", [1, 2])
@pytest.mark.parametrize("name,size", [("PX310", (W, H)), ("PX400A", (W, H)), ("PX400B", SMALL), ("TIP1000", SMALL), ("PXRET", SMALL),
                                       ("NUC201X", SMALL)])
def test_planes_and_counts_match_the_restatement(fr, renderer, name, size, aa, post):
    v = VIEWS[name]
    w, h = size
    got = _render(fr, renderer, v, aa, post, w=w, h=h)
    smp, counts = _restated(name, w, h, aa)
    _check_planes(v, got, smp, post)
    # every table radius and every level choice of the kernel, summed: equal, not close
    steps = renderer.last_deepx_phoenix_steps()
    print(name, aa, post, "steps", tuple(steps), "restated", tuple(counts))
    assert tuple(steps) == tuple(counts)
    assert counts[1] > 0


@pytest.mark.parametrize("name", ["PX400A", "NUC201X"])
def test_device_table_equals_numpy_bit_for_bit(fr, renderer, name):
    """every radius (the float's bits and the exponent), the 12 mantissas and the 2 exponents of every entry the device built"""
    v = VIEWS[name]
    w, h = SMALL
    _render(fr, renderer, v, w=w, h=h)
    orb = _orbit(name)
    want_r, want_mb, want_e = XB.table_arrays(XB.view_table(v, w, h, orb))
    n = len(want_r)
    N = len(orb[1]) - 1
    r = np.empty((n, 2), np.uint32)
    mb = np.empty((n, XB.ENTRY_DOUBLES), np.float64)
    ex = np.empty((n, 2), np.int32)
    L = fr.lib()
    got = L.fr_deepx_phoenix_bla_table(renderer._ctx, r.ctypes.data, mb.ctypes.data, ex.ctypes.data, n)
    assert got == n == (N - 1) - bin(N - 1).count("1")
    print(name, "entries", n, "r differs", int((r != want_r).any(axis=1).sum()),
          "mb differs", int((mb.view(np.uint64) != want_mb.view(np.uint64)).sum()), "exp differs", int((ex != want_e).sum()))
    assert np.array_equal(r, want_r)
    assert np.array_equal(mb.view(np.uint64), want_mb.view(np.uint64))
    assert np.array_equal(ex, want_e)
    assert L.fr_deepx_phoenix_bla_table(renderer._ctx, None, None, None, 0) == n          # NULL skips a part


@pytest.mark.parametrize("name", ["PX310", "PX400A", "PX400B", "PXRET"])
def test_iter_equals_the_unflagged_path(fr, renderer, name):
    """on every pixel (the restatements meet it alone: test_deepx_phoenix_bla_host.py)"""
    v = VIEWS[name]
    w, h = SMALL
    _, _, it_bla = _render(fr, renderer, v, w=w, h=h)
    assert renderer.last_deepx_phoenix_steps().bla > 0
    _, _, it_plain = _render(fr, renderer, v, w=w, h=h, xbla=False)
    print(name, "pixels that differ from the unflagged path", int((it_bla != it_plain).sum()))
    assert np.array_equal(it_bla, it_plain)


@pytest.mark.parametrize("name", OLD)
def test_fp64_views_as_extended_views(fr, renderer, name):
    """PA30, PA and shallowA with their zoom as a string: the flagged render equals its restatement, and iter is
    fr_render_deep_phoenix's"""
    v = VIEWS[name]
    w, h = SMALL
    got = _render(fr, renderer, v, 1, True, w=w, h=h)
    smp, counts = _restated(name, w, h, 1)
    _check_planes(v, got, smp, True)
    print(name, "steps", tuple(renderer.last_deepx_phoenix_steps()), "restated", tuple(counts))
    assert tuple(renderer.last_deepx_phoenix_steps()) == tuple(counts)
    v64 = D.VIEWS[name]
    it64 = np.empty((h, w), np.int32)
    renderer.render_deep_phoenix(fr.FractalState(zoom=v64["zoom"], max_iterations=v64["max_iter"]), w, h,
                                 fr.DeepView(v64["cx"], v64["cy"]), _ph(fr, v64), iter=it64)
    assert np.array_equal(got[2], it64), int((got[2] != it64).sum())


@pytest.mark.parametrize("max_iter", [2, 3, 4, 5, 8, 9, 16, 17, 33])
def test_short_budgets(fr, renderer, max_iter):
    """PX400A's centre with orbits of N <= 2 (no table) and of lengths at and next to powers of two: the u + 2^k <= max_iterations
    clamp and m + 2^k <= N"""
    v = dict(PX.PX400A, max_iter=max_iter)
    w, h = SMALL
    got = _render(fr, renderer, v, 1, True, w=w, h=h)
    smp, counts = XB.samples_x_bla(v, w, h)
    _check_planes(v, got, smp, True)
    print(max_iter, "steps", tuple(renderer.last_deepx_phoenix_steps()), "restated", tuple(counts))
    assert tuple(renderer.last_deepx_phoenix_steps()) == tuple(counts)


def test_shards_layouts_memory_and_async(fr, renderer):
    import torch
    v = PX.PX310
    w, h = RAGGED
    ref = _render(fr, renderer, v, 2, True, 10.0, w=w, h=h)
    ref_rgba, ref_nu, ref_it = ref
    ref_steps = renderer.last_deepx_phoenix_steps()
    assert ref_steps.bla > 0
    assert renderer.last_kernel_ms() > 0.0 and renderer.last_grid() > 0
    # host planes (FR_MEM_HOST), packed: two strip shardings, the counts of a call covering its own pixels
    for nparts, strip in ((3, None), (2, 8)):
        rgba = np.zeros_like(ref_rgba); nu = np.zeros_like(ref_nu); it = np.full_like(ref_it, -7)
        tot = np.zeros(3, np.int64)
        for part in range(nparts):
            sh = fr.Shard(part, nparts) if strip is None else fr.Shard(part, nparts, strip)
            g = sh.global_rows(h)
            a, n, i = _render(fr, renderer, v, 2, True, 10.0, shard=sh, w=w, h=h)
            rgba[g], nu[g], it[g] = a, n, i
            if sh.rows(h):
                tot += np.array(renderer.last_deepx_phoenix_steps())
        assert _same((rgba, nu, it), ref), (nparts, strip)
        assert tuple(tot) == tuple(ref_steps), (nparts, strip)
    dev = torch.device("cuda:0")
    st = _state(fr, v, 2, 10.0)
    view = _dv(fr, v)
    ph = _ph(fr, v)
    # device planes, synchronous and asynchronous on a caller's stream
    for sync in (True, False):
        d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
        d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
        d_it = torch.zeros((h, w), dtype=torch.int32, device=dev)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        if sync:
            renderer.render_deepx_phoenix(st, w, h, view, ph, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it, xbla=True)
        else:
            renderer.render_deepx_phoenix(st, w, h, view, ph, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it,
                                          stream=s.cuda_stream, sync=False, xbla=True)
            s.synchronize()
            renderer.check()
        assert renderer.last_deepx_phoenix_steps() == ref_steps, sync
        assert _same((d_rgba.cpu().numpy(), d_nu.cpu().numpy(), d_it.cpu().numpy()), ref), sync
    # FR_LAYOUT_FRAME: each of three parts writes its rows in place into whole-frame device planes
    L = fr.lib()
    p = st.to_params(fr.FractalType.Phoenix, fr.Precision.F64, True)
    p.flags |= fr.FR_FLAG_DEEPX_PHOENIX_BLA
    cv = view.to_cx()
    cph = ph.to_c()
    d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
    d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
    d_it = torch.full((h, w), -7, dtype=torch.int32, device=dev)
    o = fr._capi.fr_output(d_rgba.data_ptr(), d_nu.data_ptr(), d_it.data_ptr(), fr._capi.FR_MEM_DEVICE, fr._capi.FR_LAYOUT_FRAME)
    torch.cuda.synchronize()
    for part in range(3):
        sh = fr._capi.fr_shard(part, 3, 16)
        assert L.fr_render_deepx_phoenix(renderer._ctx, C.byref(p), C.byref(cph), C.byref(cv), w, h, C.byref(sh), C.byref(o)) == 0
    assert _same((d_rgba.cpu().numpy(), d_nu.cpu().numpy(), d_it.cpu().numpy()), ref)
    # the asynchronous form takes device planes only, with the flag as without
    host = fr._capi.fr_output(ref_rgba.ctypes.data, None, None, fr._capi.FR_MEM_HOST, 0)
    assert L.fr_render_deepx_phoenix_async(renderer._ctx, C.byref(p), C.byref(cph), C.byref(cv), w, h, None, C.byref(host), None) \
        == fr._capi.FR_ERR_INVALID_ARG


def test_counts_need_a_flagged_extended_phoenix_render(fr):
    w, h = SMALL
    with fr.Renderer(0) as r:
        out = (C.c_uint64 * 3)()
        assert fr.lib().fr_ctx_last_deepx_phoenix_steps(r._ctx, out) == fr._capi.FR_ERR_UNSUPPORTED
        with pytest.raises(fr.FractalRendererError):
            r.last_deepx_phoenix_steps()
        _render(fr, r, PX.PX310, w=w, h=h, xbla=False)
        assert fr.lib().fr_ctx_last_deepx_phoenix_steps(r._ctx, out) == fr._capi.FR_ERR_UNSUPPORTED
        _render(fr, r, PX.PX310, w=w, h=h)
        assert r.last_deepx_phoenix_steps().plain > 0
        for other in (r.last_deep_steps, r.last_deepx_steps, r.last_deep_ship_steps, r.last_deepx_ship_steps,
                      r.last_deep_julia_steps, r.last_deepx_julia_steps, r.last_deep_phoenix_steps):
            with pytest.raises(fr.FractalRendererError):
                other()                                                 # the seven other paths' counts are their own


def test_table_and_orbit_caches(fr):
    """A flagged render builds once; the same view again builds nothing; another zoom around the same centre (the same F) builds
    the table and no orbit; an unflagged render in between changes nothing; fr_render_deep_phoenix with its own flag has a table
    and counts of its own; and no other path's slot or table is touched"""
    L = fr.lib()
    v = PX.PX400A
    v2 = dict(v, zoom="2e-400", frac_bits=PX.frac_bits_of(v))
    v = dict(v, frac_bits=PX.frac_bits_of(v))
    w, h = SMALL
    with fr.Renderer(0) as r:
        fresh_plain = _render(fr, r, v, 1, True, 10.0, w=w, h=h, xbla=False)
        assert int(L.fr_deep_bla_builds(r._ctx, 1, PHOENIX)) == 0
    with fr.Renderer(0) as r:
        fresh_v2 = _render(fr, r, v2, 1, True, 10.0, w=w, h=h)
    with fr.Renderer(0) as r:
        state = lambda: (int(L.fr_deep_orbit_generation(r._ctx, 1, PHOENIX)), int(L.fr_deep_bla_builds(r._ctx, 1, PHOENIX)))
        assert state() == (0, 0)
        first = _render(fr, r, v, 1, True, 10.0, w=w, h=h)
        steps = tuple(r.last_deepx_phoenix_steps())
        assert state() == (1, 1) and steps[1] > 0
        assert _same(_render(fr, r, v, 1, True, 10.0, w=w, h=h), first) and state() == (1, 1)
        assert tuple(r.last_deepx_phoenix_steps()) == steps
        _render(fr, r, v, 2, False, w=w, h=h)                        # aa, colour and the post chain are in neither key
        assert state() == (1, 1)
        assert _same(_render(fr, r, v2, 1, True, 10.0, w=w, h=h), fresh_v2) and state() == (1, 2)
        steps2 = tuple(r.last_deepx_phoenix_steps())
        _render(fr, r, v2, 1, True, 10.0, w=w, h=h, xbla=False)      # an unflagged render in between: nothing changes
        assert state() == (1, 2)
        assert tuple(r.last_deepx_phoenix_steps()) == steps2         # ... and the counts stay the last flagged render's
        assert _same(_render(fr, r, v, 1, True, 10.0, w=w, h=h, xbla=False), fresh_plain) and state() == (1, 2)
        _render(fr, r, v, 1, True, 10.0, w=W, h=H)                   # another frame shape: another dcmax
        assert state() == (1, 3)
        assert _same(_render(fr, r, v, 1, True, 10.0, w=w, h=h), first) and state() == (1, 4)
        assert tuple(r.last_deepx_phoenix_steps()) == steps
        # fr_render_deep_phoenix with FR_FLAG_DEEP_PHOENIX_BLA: the fp64 slot, its table and its counts
        v64 = D.PA30
        it64 = np.empty((h, w), np.int32)
        r.render_deep_phoenix(fr.FractalState(zoom=v64["zoom"], max_iterations=v64["max_iter"]), w, h,
                              fr.DeepView(v64["cx"], v64["cy"]), _ph(fr, v64), iter=it64, bla=True)
        assert state() == (1, 4)
        assert int(L.fr_deep_orbit_generation(r._ctx, 0, PHOENIX)) == 1 and int(L.fr_deep_bla_builds(r._ctx, 0, PHOENIX)) == 1
        assert tuple(r.last_deepx_phoenix_steps()) == steps and tuple(r.last_deep_phoenix_steps()) != steps
        assert _same(_render(fr, r, v, 1, True, 10.0, w=w, h=h), first) and state() == (1, 4)
        for x, f in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)):
            assert int(L.fr_deep_orbit_generation(r._ctx, x, f)) == 0 and int(L.fr_deep_bla_builds(r._ctx, x, f)) == 0, (x, f)
