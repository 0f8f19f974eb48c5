"""Deep Burning Ship views with bilinear approximation on the GPU (fr_render_deep_ship with FR_FLAG_DEEP_SHIP_BLA): the planes
and the step counts against the numpy restatement (tests/deep_ship_bla_ref.py), the device-built table against numpy's, the
direct fixed-point iteration, the unflagged path, a real-axis view, short budgets, shards, layouts, memory kinds, the
asynchronous form, the caches of one context, and the other entry points' indifference to the flag."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_ref as R
import deep_ship_bla_ref as SB
import deep_ship_ref as S
from test_deep_ship_gpu import NU_TOL, RGB_TOL, _few, _same

pytestmark = pytest.mark.gpu

W, H = 256, 192
REAL_AXIS = dict(cx="-1.75", cy="0", zoom=1e-20, max_iter=500)


def _state(fr, v, aa=1):
    return fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"], antialiasing_samples=aa)


def _render(fr, r, v, aa=1, post=False, shard=None, w=W, h=H, bla=True):
    rows = shard.rows(h) if shard else h
    rgba = np.empty((rows, w, 4), np.float32)
    nu = np.empty((rows, w), np.float64)
    it = np.empty((rows, w), np.int32)
    r.render_deep_ship(_state(fr, v, aa), w, h, fr.DeepView(v["cx"], v["cy"]), post_chain=post, rgba=rgba, nu=nu, iter=it,
                       shard=shard, bla=bla)
    return rgba, nu, it


@functools.lru_cache(maxsize=None)
def _restated(name, aa):
    """computed once per (view, aa), shared, never changed"""
    return SB.restate_bla(S.VIEWS[name], W, H, aa)


def _expected_rgba(oracle, v, samples, aa, post):
    """the colour stage of the fp64 Burning Ship path on the restated samples, at the samples' own frame size: per-sample
    colour (interior black), the aa average in the shader's order, then the post chain with the Burning Ship floors"""
    h, w = samples[0][0].shape
    p = oracle.OracleParams(fractal=2, max_iterations=v["max_iter"], zoom=v["zoom"], aa=aa, post_chain=0)
    acc = np.zeros((h, w, 3), np.float32)
    for it, r2 in samples:
        acc = acc + oracle.colorize(p, S.smooth(it, r2, v["max_iter"]))[..., :3]
    if aa > 1:
        acc = acc / np.float32(aa * aa)
    if post:
        acc = np.array([oracle.post_chain(c, julia_floors=1) for c in acc.reshape(-1, 3)], np.float32).reshape(h, w, 3)
    return acc


def _check_planes(oracle, v, got, samples, aa, post):
    rgba, nu, it = got
    r_it, r_r2 = samples[0]
    print("iter mismatches", int((it != r_it).sum()), "of", it.size)
    assert np.array_equal(it, r_it), int((it != r_it).sum())
    dnu = np.abs(nu - S.smooth(r_it, r_r2, v["max_iter"])).max()
    print("max |dnu|", dnu)
    assert dnu <= NU_TOL
    assert np.all(rgba[..., 3] == 1.0)
    bad = np.abs(rgba[..., :3] - _expected_rgba(oracle, v, samples, aa, post)).max(axis=2) > RGB_TOL
    print("rgb over tolerance", int(bad.sum()))
    assert _few(bad, it.size), int(bad.sum())


@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("aa", [1, 2])
@pytest.mark.parametrize("name", ["shallow", "needle", "A", "B"])
def test_planes_and_counts_match_the_restatement(fr, renderer, oracle, name, aa, post):
    v = S.VIEWS[name]
    got = _render(fr, renderer, v, aa, post)
    samples, counts = _restated(name, aa)
    _check_planes(oracle, v, got, samples, aa, post)
    # every table radius and every level choice of the kernel, summed: equal, not close
    steps = renderer.last_deep_ship_steps()
    print(name, aa, post, "steps", tuple(steps), "restated", tuple(counts))
    assert tuple(steps) == tuple(counts)
    if name in ("A", "B"):
        assert counts[1] > 0
    else:
        assert counts[1] == 0


@pytest.mark.parametrize("name", ["A", "B"])
def test_device_table_equals_numpy_bit_for_bit(fr, renderer, name):
    """every (A, B, r) the device built, through its sqrt included, against bla_table"""
    v = S.VIEWS[name]
    _render(fr, renderer, v)
    orb = S.reference_orbit(v["cx"], v["cy"], v["zoom"], v["max_iter"])
    tab = SB.bla_table(orb, SB.dcmax(W, H, v["zoom"]))
    n = sum(len(T["r"]) for T in tab)
    r = np.empty(n, np.float64)
    ab = np.empty((n, 8), np.float64)
    got = fr.lib().fr_deep_ship_bla_table(renderer._ctx, r.ctypes.data, ab.ctypes.data, n)
    assert got == n == (len(orb) - 2) - bin(len(orb) - 2).count("1")
    want_r = np.concatenate([T["r"] for T in tab])
    want_ab = np.concatenate([np.stack([T[q] for q in SB.ELEMS], axis=1) for T in tab])
    print(name, "entries", n, "r differs", int((r.view(np.uint64) != want_r.view(np.uint64)).sum()),
          "ab differs", int((ab.view(np.uint64) != want_ab.view(np.uint64)).sum()))
    assert np.array_equal(r.view(np.uint64), want_r.view(np.uint64))
    assert np.array_equal(ab.view(np.uint64), want_ab.view(np.uint64))


@pytest.mark.parametrize("name", ["A", "B"])
def test_bla_is_exact_where_fp64_collapses(fr, renderer, name):
    """256 random pixels against the direct fixed-point iteration (the restatement alone gives 1.0)"""
    v = S.VIEWS[name]
    _, _, it = _render(fr, renderer, v)
    rng = np.random.default_rng(99)
    ys, xs = rng.integers(0, H, 256), rng.integers(0, W, 256)
    ex = np.array([S.exact_iter(v["cx"], v["cy"], int(x), int(y), W, H, v["zoom"], v["max_iter"]) for x, y in zip(xs, ys)])
    agreement = (it[ys, xs] == ex).mean()
    print(name, "agreement with the exact iteration", agreement)
    assert agreement >= 0.99


@pytest.mark.parametrize("name,bar", [("shallow", 1.0), ("needle", 1.0), ("A", 0.999), ("B", 0.999)])
def test_agreement_with_the_unflagged_path(fr, renderer, name, bar):
    """Share of pixels whose iter equals the unflagged path's on the same context.  The restatements give 1.0 on the shallow
    views (no BLA step) and on A, and 0.99953 on B (23 pixels of 49152: an escape inside a skipped stretch or a rounding
    away).  The bar on the deep views, 0.999, is 49 such pixels."""
    v = S.VIEWS[name]
    _, _, it_bla = _render(fr, renderer, v)
    _, _, it_plain = _render(fr, renderer, v, bla=False)
    share = (it_bla == it_plain).mean()
    print(name, "agreement with the unflagged path", share)
    assert share >= bar


def test_real_axis_view_takes_no_bla_step(fr, renderer):
    """cy = "0": Y = 0 on the whole orbit, the fold condition makes every r 0"""
    got = _render(fr, renderer, REAL_AXIS, 2, True, w=64, h=48)
    steps = renderer.last_deep_ship_steps()
    assert steps.plain > 0 and tuple(steps)[1:] == (0, 0)
    assert _same(got, _render(fr, renderer, REAL_AXIS, 2, True, w=64, h=48, bla=False))


@pytest.mark.parametrize("max_iter", [2, 3, 4, 5, 8, 9, 16, 17, 33])
def test_short_budgets(fr, renderer, oracle, max_iter):
    """view B's centre with orbits of N <= 2 (no table) and of lengths at and next to powers of two"""
    v = dict(S.SHIP_B, max_iter=max_iter)
    w, h = 64, 48
    got = _render(fr, renderer, v, 1, True, w=w, h=h)
    samples, counts = SB.restate_bla(v, w, h)
    _check_planes(oracle, v, got, samples, 1, True)
    print(max_iter, "steps", tuple(renderer.last_deep_ship_steps()), "restated", tuple(counts))
    assert tuple(renderer.last_deep_ship_steps()) == tuple(counts)


def test_shards_layouts_memory_and_async(fr, renderer):
    import torch
    v = S.SHIP_B
    w, h = 203, 117
    ref = _render(fr, renderer, v, 2, True, w=w, h=h)
    ref_rgba, ref_nu, ref_it = ref
    ref_steps = renderer.last_deep_ship_steps()
    assert ref_steps.bla > 0
    assert renderer.last_kernel_ms() > 0.0 and renderer.last_grid() > 0
    for nparts in (1, 3, 8):
        rgba = np.zeros_like(ref_rgba); nu = np.zeros_like(ref_nu); it = np.full_like(ref_it, -7)
        tot = np.zeros(3, np.int64)
        for part in range(nparts):
            sh = fr.Shard(part, nparts)
            g = sh.global_rows(h)
            a, n, i = _render(fr, renderer, v, 2, True, shard=sh, w=w, h=h)
            rgba[g], nu[g], it[g] = a, n, i
            if sh.rows(h):
                tot += np.array(renderer.last_deep_ship_steps())
        assert _same((rgba, nu, it), ref), nparts
        assert tuple(tot) == tuple(ref_steps), nparts                   # the counts of a call cover its own pixels
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
            renderer.render_deep_ship(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it, bla=True)
        else:
            renderer.render_deep_ship(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it,
                                      stream=s.cuda_stream, sync=False, bla=True)
            s.synchronize()
            renderer.check()
        assert renderer.last_deep_ship_steps() == ref_steps, sync
        assert _same((d_rgba.cpu().numpy(), d_nu.cpu().numpy(), d_it.cpu().numpy()), ref), sync
    # FR_LAYOUT_FRAME: each part writes its rows in place into whole-frame device planes
    L = fr.lib()
    p = st.to_params(fr.FractalType.BurningShip, fr.Precision.F64, True)
    p.flags |= fr.FR_FLAG_DEEP_SHIP_BLA
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


def test_counts_need_a_flagged_ship_render(fr):
    with fr.Renderer(0) as r:
        with pytest.raises(fr.FractalRendererError):
            r.last_deep_ship_steps()
        _render(fr, r, S.SHIP_A, w=64, h=48, bla=False)
        with pytest.raises(fr.FractalRendererError):
            r.last_deep_ship_steps()
        _render(fr, r, S.SHIP_A, w=64, h=48)
        assert r.last_deep_ship_steps().plain > 0
        with pytest.raises(fr.FractalRendererError):
            r.last_deep_steps()                                         # the Mandelbrot path's counts are its own


def test_caches_across_paths(fr):
    """Flagged and unflagged ship renders of one view, a zoom change at a fixed centre (the table is rebuilt, the orbit
    kept), another ship view, a flagged Mandelbrot render and a Deep_Zoom render on one context: every frame equals the same
    frame rendered alone, and each path's counts stay its own"""
    W2, H2 = 160, 120
    vb2 = dict(S.SHIP_B, zoom=2e-100)

    def ship(r, v, bla):
        out = _render(fr, r, v, 1, True, w=W2, h=H2, bla=bla)
        return out + ((tuple(r.last_deep_ship_steps()),) if bla else ())

    def mandelbrot(r):
        v = R.VIEW_B
        rgba = np.empty((H2, W2, 4), np.float32)
        nu = np.empty((H2, W2), np.float64)
        it = np.empty((H2, W2), np.int32)
        r.render_deep(_state(fr, v), W2, H2, fr.DeepView(v["cx"], v["cy"]), post_chain=True, rgba=rgba, nu=nu, iter=it, bla=True)
        return rgba, nu, it, tuple(r.last_deep_steps())

    def deep_zoom(r):
        st = fr.FractalState(center_x=-0.743643887037151, center_y=0.131825904205330, zoom=1e-5, max_iterations=512,
                             use_perturbation=True)
        rgba = np.empty((H2, W2, 4), np.float32)
        it = np.empty((H2, W2), np.int32)
        r.render(st, W2, H2, fractal_type=fr.FractalType.Deep_Zoom, precision=fr.Precision.F32, rgba=rgba, iter=it)
        return rgba, it

    jobs = {"Bb": lambda r: ship(r, S.SHIP_B, True), "Bp": lambda r: ship(r, S.SHIP_B, False),
            "B2b": lambda r: ship(r, vb2, True), "Ab": lambda r: ship(r, S.SHIP_A, True),
            "Ap": lambda r: ship(r, S.SHIP_A, False), "Mb": mandelbrot, "dz": deep_zoom}
    alone = {}
    for key, fn in jobs.items():
        with fr.Renderer(0) as r:
            alone[key] = fn(r)
    assert alone["Bb"][3][1] > 0 and alone["Mb"][3][1] > 0
    with fr.Renderer(0) as r:
        ship_steps = mand_steps = None
        for key in ("Bb", "Bp", "Bb", "B2b", "Bb", "Mb", "dz", "Ab", "Bp", "Ap", "B2b", "Mb", "dz", "Bb"):
            got = jobs[key](r)
            for g, want in zip(got, alone[key]):
                assert np.array_equal(np.asarray(g).view(np.uint8), np.asarray(want).view(np.uint8)), key
            if key in ("Bb", "B2b", "Ab"):
                ship_steps = got[3]
            if key == "Mb":
                mand_steps = got[3]
            # a render of one path leaves the other path's counts alone
            if ship_steps is not None:
                assert tuple(r.last_deep_ship_steps()) == ship_steps, key
            if mand_steps is not None:
                assert tuple(r.last_deep_steps()) == mand_steps, key


def test_other_entry_points_ignore_the_flag(fr, renderer):
    """fr_render, fr_render_deep and fr_render_deepx given 0x8 write the bytes they write without it"""
    L, E = fr.lib(), fr._capi
    w, h = 64, 48

    def planes():
        rgba = np.zeros((h, w, 4), np.float32)
        nu = np.zeros((h, w), np.float64)
        it = np.zeros((h, w), np.int32)
        return (rgba, nu, it), E.fr_output(rgba.ctypes.data, nu.ctypes.data, it.ctypes.data, E.FR_MEM_HOST, 0)

    def both(call, p):
        out = []
        for extra in (0, E.FR_FLAG_DEEP_SHIP_BLA):
            p.flags = E.FR_FLAG_POST_CHAIN | extra
            arrays, o = planes()
            assert call(p, o) == E.FR_OK, L.fr_last_error()
            out.append(arrays)
        assert _same(out[1], out[0])
        assert out[0][2].any()

    for ftype in (fr.FractalType.Mandelbrot, fr.FractalType.BurningShip):
        p = fr.FractalState(max_iterations=200).to_params(ftype, fr.Precision.F64)
        both(lambda p, o: L.fr_render(renderer._ctx, C.byref(p), w, h, C.byref(o)), p)
    v = R.VIEW_A
    p = _state(fr, v).to_params(fr.FractalType.Mandelbrot, fr.Precision.F64)
    cv = fr.DeepView(v["cx"], v["cy"]).to_c()
    both(lambda p, o: L.fr_render_deep(renderer._ctx, C.byref(p), C.byref(cv), w, h, None, C.byref(o)), p)
    cx = fr.DeepView(v["cx"], v["cy"], zoom=repr(v["zoom"])).to_cx()
    both(lambda p, o: L.fr_render_deepx(renderer._ctx, C.byref(p), C.byref(cx), w, h, None, C.byref(o)), p)
    # and the ship's counts are not theirs to change
    _render(fr, renderer, S.SHIP_A, w=w, h=h)
    steps = renderer.last_deep_ship_steps()
    both(lambda p, o: L.fr_render_deep(renderer._ctx, C.byref(p), C.byref(cv), w, h, None, C.byref(o)), p)
    assert renderer.last_deep_ship_steps() == steps
