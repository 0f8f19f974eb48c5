"""Deep Burning Ship views with extended-exponent deltas on the GPU (fr_render_deepx_ship): the bytes of fr_render_deep_ship
on views a double holds, the numpy restatement of the two-mode ship step on views it does not (structured views, the tip
of the needle where Y = 0 exactly, a nucleus whose orbit returns to 2^-1128), the direct fixed-point iteration, shards,
layouts, memory kinds, the asynchronous form, the four orbit slots of one context, and every rejected call."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_ref as R
import deep_ship_ref as S
import deepx_ref as X
import deepx_ship_ref as SX

pytestmark = pytest.mark.gpu

V = SX.views()
RGB_TOL = 1e-4                          # test_deep_ship_gpu.py's tolerances
NU_TOL = 1e-9


def _few(bad, n):
    """palette wrap exceptions: a sample whose t sits on a knot or on fract's wrap may take the neighbouring colour"""
    return int(bad.sum()) <= max(2, int(0.001 * n))


def _state(fr, v, aa=1):
    return fr.FractalState(max_iterations=v["max_iter"], antialiasing_samples=aa)


def _view(fr, v):
    return fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"])


def _render(fr, r, v, w, h, aa=1, post=False, shard=None):
    rows = shard.rows(h) if shard else h
    rgba = np.empty((rows, w, 4), np.float32)
    nu = np.empty((rows, w), np.float64)
    it = np.empty((rows, w), np.int32)
    r.render_deepx_ship(_state(fr, v, aa), w, h, _view(fr, v), post_chain=post, rgba=rgba, nu=nu, iter=it, shard=shard)
    return rgba, nu, it


def _same(got, want):
    return all(np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)) for g, w in zip(got, want))


# ---- 1. views a double holds: the bytes of fr_render_deep_ship ------------------------------------------------------------
@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("aa", [1, 2])
@pytest.mark.parametrize("name", ["A", "B"])
def test_views_a_double_holds_get_the_bytes_of_fr_render_deep_ship(fr, renderer, name, aa, post):
    w, h = 256, 192
    v = S.VIEWS[name]
    got = _render(fr, renderer, SX.as_x_view(v), w, h, aa, post)
    want = (np.empty((h, w, 4), np.float32), np.empty((h, w), np.float64), np.empty((h, w), np.int32))
    renderer.render_deep_ship(fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"], antialiasing_samples=aa), w, h,
                              fr.DeepView(v["cx"], v["cy"]), post_chain=post, rgba=want[0], nu=want[1], iter=want[2])
    for k, g, x in zip(("rgba", "nu", "iter"), got, want):
        assert _same((g,), (x,)), (k, int((g != x).sum()))
    assert len(np.unique(want[2])) >= 40


# ---- 2. against the restatement ---------------------------------------------------------------------------------------------
FRAMES = {                              # name: (view, W, H, aa, post, rows)
    "S400": ("S400", 128, 96, 1, False, None),
    "S400-aa2-post": ("S400", 128, 96, 2, True, None),
    "S310": ("S310", 128, 96, 1, False, None),
    "TIP400": ("TIP400", 48, 36, 1, False, None),
    "TIP1000-band": ("TIP1000", 48, 36, 1, False, tuple(range(12, 24))),
    "TIPY300": ("TIPY300", 48, 36, 1, False, None),
}


@functools.lru_cache(maxsize=None)
def _restated(case):
    """computed once per frame, shared, never changed: the samples and the restatement's step counts"""
    name, w, h, aa, _, rows = FRAMES[case]
    stats = {}
    return SX.restate_ship_x(V[name], w, h, aa, rows=None if rows is None else list(rows), stats=stats), stats


def _expected_rgb(oracle, v, samples, aa, post):
    """the colour stage of the fp64 Burning Ship path on the restated samples (test_deep_ship_gpu.py's)"""
    p = oracle.OracleParams(fractal=2, max_iterations=v["max_iter"], zoom=1.0, aa=aa, post_chain=0)
    acc = np.zeros(samples[0][0].shape + (3,), np.float32)
    for it, r2 in samples:
        acc = acc + oracle.colorize(p, S.smooth(it, r2, v["max_iter"]))[..., :3]
    if aa > 1:
        acc = acc / np.float32(aa * aa)
    if post:
        shape = acc.shape
        acc = np.array([oracle.post_chain(c, julia_floors=1) for c in acc.reshape(-1, 3)], np.float32).reshape(shape)
    return acc


@pytest.mark.parametrize("case", list(FRAMES))
def test_planes_match_the_restatement(fr, renderer, oracle, case):
    name, w, h, aa, post, rows = FRAMES[case]
    v = V[name]
    samples, stats = _restated(case)
    rgba, nu, it = _render(fr, renderer, v, w, h, aa, post)
    if rows is not None:
        rgba, nu, it = rgba[list(rows)], nu[list(rows)], it[list(rows)]
    r_it, r_r2 = samples[0]
    print(case, stats, "iter mismatches", int((it != r_it).sum()), "escaped", float((r_it < v["max_iter"]).mean()),
          "distinct", len(np.unique(r_it)))
    assert stats["ext_steps"] > stats["plain_steps"] and stats["to_plain"] > 0, stats
    # An extended fold flips only where an orbit coordinate lies below the delta, that is below 2^-400.  The orbits of S310 and
    # S400 never come that close to an axis (the restatement counts 0 flips on their frames).  The tip's Y = 0 flips once per
    # sample with b < 0, in its first extended step (864 on this frame at either depth) -- with X = 0, so d = 2X + b = b and
    # the 2X term is not seen.  TIPY300 is the frame that sees it: Y is stored nonzero, 2^-1000 below X, 480 extended flips
    # meet it, and tests/test_deepx_ship_host.py shows that a fold forming d = X + a changes 208 of this frame's 1728 iter.
    assert (stats["flipped_ext"] > 0) == name.startswith("TIP"), stats
    assert np.array_equal(it, r_it), int((it != r_it).sum())
    dnu = np.abs(nu - S.smooth(r_it, r_r2, v["max_iter"])).max()
    print("max |dnu|", dnu)
    assert dnu <= NU_TOL
    assert np.all(rgba[..., 3] == 1.0)
    d = np.abs(rgba[..., :3] - _expected_rgb(oracle, v, samples, aa, post)).max(axis=2)
    bad = d > RGB_TOL
    print("rgb over tolerance", int(bad.sum()), "median", float(np.median(d)))
    assert _few(bad, it.size), int(bad.sum())
    if aa == 1 and not post:
        assert np.all(rgba[..., :3][r_it == v["max_iter"]] == 0.0)                    # interior samples are black


# ---- 3. against the exact iteration -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S310", "S400"])
def test_structured_views_agree_with_the_exact_iteration(fr, renderer, name):
    g = SX.exact_golden()
    v, ex = V[name], g[name]
    _, _, it = _render(fr, renderer, v, 128, 96)
    largest = np.unique(ex, return_counts=True)[1].max() / len(ex)
    agreement = (it[g["ys"], g["xs"]] == ex).mean()
    print(name, "largest exact class", largest, "agreement", agreement)
    assert largest <= 0.60                            # a collapsed frame cannot agree by chance
    assert agreement >= 0.99


# ---- 4. the nucleus -----------------------------------------------------------------------------------------------------------
def test_nucleus_view_is_interior(fr, renderer):
    """Centred on the period-546 nucleus the orbit returns to 2^-1128 -- points only the extended storage holds -- and every
    sample of the view is interior, as the exact iteration says.  What this checks is that the extended step, run for 1200
    updates with no plain step before the last, produces no false escape around such points.  It does NOT pin the fold: almost
    all of the restatement's 2332 flipped steps here are at Z_0 = 0 after a rebase, and a fold that never flipped in extended
    mode would leave the view interior too.  The flipped branch is pinned by the TIPY300 frame above."""
    v = V["NUC546"]
    rgba, nu, it = _render(fr, renderer, v, 48, 36)
    assert np.all(it == v["max_iter"]), int((it != v["max_iter"]).sum())
    assert np.all(nu == float(v["max_iter"])) and np.all(rgba[..., :3] == 0.0)


# ---- 5. shards, layouts, memory kinds, the asynchronous form ------------------------------------------------------------------
def test_shards_layouts_memory_and_async(fr, renderer):
    import torch
    v = V["S400"]
    w, h = 203, 117
    ref = _render(fr, renderer, v, w, h, 2, True)
    ref_rgba, ref_nu, ref_it = ref
    assert renderer.last_kernel_ms() > 0.0 and renderer.last_grid() > 0
    assert _same(_render(fr, renderer, v, w, h, 2, True), ref)                        # twice: identical bytes
    assert len(np.unique(ref_it)) > 5
    for nparts, strip in ((1, None), (3, None), (3, 8), (8, None)):
        rgba = np.zeros_like(ref_rgba); nu = np.zeros_like(ref_nu); it = np.full_like(ref_it, -7)
        for part in range(nparts):
            sh = fr.Shard(part, nparts) if strip is None else fr.Shard(part, nparts, strip)
            g = sh.global_rows(h)
            a, n, i = _render(fr, renderer, v, w, h, 2, True, shard=sh)
            rgba[g], nu[g], it[g] = a, n, i
        assert _same((rgba, nu, it), ref), (nparts, strip)
    dev = torch.device("cuda:0")
    st = _state(fr, v, 2)
    view = _view(fr, v)
    # device planes, synchronous and asynchronous on a caller's stream
    for sync in (True, False):
        d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
        d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
        d_it = torch.zeros((h, w), dtype=torch.int32, device=dev)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        if sync:
            renderer.render_deepx_ship(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it)
        else:
            renderer.render_deepx_ship(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it,
                                       stream=s.cuda_stream, sync=False)
            s.synchronize()
            renderer.check()
        assert _same((d_rgba.cpu().numpy(), d_nu.cpu().numpy(), d_it.cpu().numpy()), ref), sync
    # FR_LAYOUT_FRAME: each part writes its rows in place into whole-frame device planes
    L = fr.lib()
    p = st.to_params(fr.FractalType.BurningShip, fr.Precision.F64, True)
    cv = view.to_cx()
    for nparts in (3, 8):
        d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
        d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
        d_it = torch.full((h, w), -7, dtype=torch.int32, device=dev)
        o = fr._capi.fr_output(d_rgba.data_ptr(), d_nu.data_ptr(), d_it.data_ptr(), fr._capi.FR_MEM_DEVICE,
                               fr._capi.FR_LAYOUT_FRAME)
        torch.cuda.synchronize()
        for part in range(nparts):
            sh = fr._capi.fr_shard(part, nparts, 16 if nparts == 3 else 0)
            assert L.fr_render_deepx_ship(renderer._ctx, C.byref(p), C.byref(cv), w, h, C.byref(sh), C.byref(o)) == 0
        assert _same((d_rgba.cpu().numpy(), d_nu.cpu().numpy(), d_it.cpu().numpy()), ref), nparts
    # the asynchronous form takes device planes only
    host = fr._capi.fr_output(ref_rgba.ctypes.data, None, None, fr._capi.FR_MEM_HOST, 0)
    assert L.fr_render_deepx_ship_async(renderer._ctx, C.byref(p), C.byref(cv), w, h, None, C.byref(host), None) \
        == fr._capi.FR_ERR_INVALID_ARG


# ---- 6. the four orbit slots of one context -------------------------------------------------------------------------------------
def test_four_orbit_slots_do_not_evict_each_other(fr):
    w, h = 96, 72
    XV = X.views()

    def shipx(r, v=None):
        return _render(fr, r, v or V["S400"], w, h, 1, True)

    def ship(r):
        v = S.SHIP_A
        out = (np.empty((h, w, 4), np.float32), np.empty((h, w), np.float64), np.empty((h, w), np.int32))
        r.render_deep_ship(fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"]), w, h, fr.DeepView(v["cx"], v["cy"]),
                           post_chain=True, rgba=out[0], nu=out[1], iter=out[2])
        return out

    def deepx(r):
        v = XV["T300"]
        out = (np.empty((h, w, 4), np.float32), np.empty((h, w), np.float64), np.empty((h, w), np.int32))
        r.render_deep(fr.FractalState(max_iterations=v["max_iter"]), w, h, fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"]),
                      post_chain=True, rgba=out[0], nu=out[1], iter=out[2])
        return out

    def deep(r):
        v = R.VIEW_A
        out = (np.empty((h, w, 4), np.float32), np.empty((h, w), np.float64), np.empty((h, w), np.int32))
        r.render_deep(fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"]), w, h, fr.DeepView(v["cx"], v["cy"]),
                      post_chain=True, rgba=out[0], nu=out[1], iter=out[2])
        return out

    paths = dict(shipx=shipx, ship=ship, deepx=deepx, deep=deep)
    alone = {}
    for k, f in paths.items():
        with fr.Renderer(0) as r:
            alone[k] = f(r)
    assert not _same(alone["shipx"], alone["deepx"])
    with fr.Renderer(0) as r:
        for k in ("shipx", "ship", "deepx", "deep", "shipx", "deepx", "ship", "deep", "shipx"):
            assert _same(paths[k](r), alone[k]), k
        shipx(r, V["TIP400"])                                  # another extended ship view: that slot alone changes
        for k in ("deep", "deepx", "ship", "shipx"):
            assert _same(paths[k](r), alone[k]), k


# ---- 7. unsupported and invalid calls -------------------------------------------------------------------------------------------
def test_unsupported_and_invalid_calls(fr, renderer):
    L, K = fr.lib(), fr._capi
    E, U = K.FR_ERR_INVALID_ARG, K.FR_ERR_UNSUPPORTED
    ship, f64 = fr.FractalType.BurningShip, fr.Precision.F64
    rgba = np.zeros((8, 8, 4), np.float32)
    o = K.fr_output(rgba.ctypes.data, None, None, K.FR_MEM_HOST, 0)

    def call(p, zoom="1e-400", frac_bits=0, reserved=0):
        v = K.fr_deepx_view(b"-2", b"0", zoom.encode(), frac_bits, reserved)
        return L.fr_render_deepx_ship(renderer._ctx, C.byref(p), C.byref(v), 8, 8, None, C.byref(o))

    def params(ftype=ship, prec=f64, flags=0, **kw):
        p = fr.FractalState(max_iterations=64, **kw).to_params(ftype, prec, False)
        p.flags |= flags
        return p

    assert call(params()) == 0 and np.all(rgba[..., 3] == 1.0)
    for flag in (K.FR_FLAG_DEEP_BLA, K.FR_FLAG_DEEPX_BLA, K.FR_FLAG_DEEP_SHIP_BLA):
        assert call(params(flags=flag)) == U, flag
    assert call(params(ftype=fr.FractalType.Mandelbrot)) == U
    assert call(params(prec=fr.Precision.F32)) == U
    assert call(params(orbit_trap_enabled=True)) == U
    assert call(params(interior_style=3)) == U
    for z in ("1e-1001", "2e3", "z"):
        assert call(params(), zoom=z) == E, z
    assert call(params(), frac_bits=100) == E
    assert call(params(), reserved=1) == E
    with pytest.raises(ValueError):
        renderer.render_deepx_ship(fr.FractalState(), 8, 8, fr.DeepView("-2", "0"), rgba=rgba)
    with pytest.raises(ValueError):                               # tests/test_deep_ship_host.py pins this one too
        renderer.render_deep_ship(fr.FractalState(), 8, 8, fr.DeepView("-2", "0", zoom="1e-400"), rgba=rgba)
