"""Extended Burning Ship views with bilinear approximation on the GPU (fr_render_deepx_ship with FR_FLAG_DEEPX_SHIP_BLA): the
planes and the step counts against the numpy restatement (tests/deepx_ship_bla_ref.py), the device-built table against
numpy's bit for bit, the direct fixed-point iteration, fr_render_deep_ship's fp64 BLA where both can render a view, the
unflagged path, edge cases, shards, layouts, memory kinds, the asynchronous form, the caches of one context, the other entry
points' indifference to the flag, and a ship sequence with the flag."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_ref as R
import deep_ship_bla_ref as SB
import deep_ship_ref as S
import deepx_ref as X
import deepx_ship_bla_ref as XB
import deepx_ship_ref as SX
from test_deepx_ship_bla_host import EQUAL_TO_UNFLAGGED
from test_deepx_ship_gpu import NU_TOL, RGB_TOL, _expected_rgb, _few, _same

pytestmark = pytest.mark.gpu

V = SX.views()
FRAMES = {                              # case: (view, W, H, aa, post)
    "S400": ("S400", 128, 96, 1, False),
    "S400-aa2-post": ("S400", 128, 96, 2, True),
    "S310": ("S310", 128, 96, 1, False),
    "NUC546": ("NUC546", 128, 96, 1, False),
    "TIPY300": ("TIPY300", 48, 36, 1, False),
}


def _render(fr, r, v, w, h, aa=1, post=False, shard=None, bla=True):
    rows = shard.rows(h) if shard else h
    rgba = np.empty((rows, w, 4), np.float32)
    nu = np.empty((rows, w), np.float64)
    it = np.empty((rows, w), np.int32)
    r.render_deepx_ship(fr.FractalState(max_iterations=v["max_iter"], antialiasing_samples=aa), w, h,
                        fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"], frac_bits=v.get("frac_bits", 0)), post_chain=post,
                        rgba=rgba, nu=nu, iter=it, shard=shard, bla=bla)
    return rgba, nu, it


@functools.lru_cache(maxsize=None)
def _orbit(name):
    return SX.orbit_of(V[name])


@functools.lru_cache(maxsize=None)
def _restated(case):
    """computed once per frame, shared, never changed: the samples and the three counts"""
    name, w, h, aa, _ = FRAMES[case]
    return XB.restate_ship_x_bla(V[name], w, h, aa, orbit=_orbit(name))


@functools.lru_cache(maxsize=None)
def _unflagged(name):
    return SX.restate_ship_x(V[name], 128, 96, orbit=_orbit(name))


def _check_planes(oracle, v, got, samples, aa, post):
    rgba, nu, it = got
    r_it, r_r2 = samples[0]
    ndiff = int((it != r_it).sum())
    dnu = float(np.abs(nu - S.smooth(r_it, r_r2, v["max_iter"])).max())
    bad = np.abs(rgba[..., :3] - _expected_rgb(oracle, v, samples, aa, post)).max(axis=2) > RGB_TOL
    print("iter differences", ndiff, "max |nu - restated|", dnu, "rgb outside tolerance", int(bad.sum()), "of", it.size)
    assert ndiff == 0
    assert dnu <= NU_TOL
    assert np.all(rgba[..., 3] == 1.0)
    assert _few(bad, it.size), int(bad.sum())


# 1. planes and counts equal the restatement
@pytest.mark.parametrize("case", list(FRAMES))
def test_planes_and_counts_match_the_restatement(fr, renderer, oracle, case):
    """Restated counts (single steps, BLA steps, updates skipped): S400 [1788676, 70518, 31722444], at aa 2
    [7152221, 282084, 126889168], S310 [1791263, 97629, 24506016], NUC546 [73724, 233460, 14671876], TIPY300
    [752459, 2858, 115064]."""
    name, w, h, aa, post = FRAMES[case]
    v = V[name]
    got = _render(fr, renderer, v, w, h, aa, post)
    steps = tuple(renderer.last_deepx_ship_steps())
    samples, counts = _restated(case)
    print(case, "counts", steps, "restated", tuple(counts))
    _check_planes(oracle, v, got, samples, aa, post)
    # every table radius and every level choice of the kernel, summed over the whole frame: equal, not close
    assert steps == tuple(counts)
    assert counts[1] > 0
    if name == "TIPY300":                                          # the fold cap on a coordinate 2^-1000 below its partner:
        assert 0 < counts[2] < counts[0]                           # few BLA steps, but not none
    else:
        assert counts[2] > counts[0]


# 2. the device table, through its sqrt and division included
@pytest.mark.parametrize("name,w,h", [("S400", 128, 96), ("TIPY300", 48, 36)])
def test_device_table_equals_numpy_bit_for_bit(fr, renderer, name, w, h):
    v = V[name]
    _render(fr, renderer, v, w, h)
    tab = XB.table_of(v, w, h, _orbit(name))
    n = sum(len(T["rv"]) for T in tab)
    r = np.empty(n, np.dtype([("v", np.float32), ("e", np.int32)]))
    ab = np.empty((n, 8), np.float64)
    abe = np.empty((n, 2), np.int32)
    L = fr.lib()
    assert L.fr_deepx_ship_bla_table(renderer._ctx, None, None, None, 0) == n
    assert L.fr_deepx_ship_bla_table(renderer._ctx, r.ctypes.data, ab.ctypes.data, abe.ctypes.data, n) == n
    want_rv = np.concatenate([T["rv"] for T in tab]).astype(np.float32)
    want_re = np.concatenate([T["re"] for T in tab]).astype(np.int32)
    want_ab = np.concatenate([np.stack([T[q] for q in XB.ELEMS], axis=1) for T in tab])
    want_abe = np.concatenate([np.stack([T["ea"], T["eb"]], axis=1) for T in tab]).astype(np.int32)
    assert np.array_equal(r["v"].view(np.uint32), want_rv.view(np.uint32)) and np.array_equal(r["e"], want_re)
    assert np.array_equal(ab.view(np.uint64), want_ab.view(np.uint64))
    assert np.array_equal(abe, want_abe)
    assert (r["v"] > 0).sum() > n // 2


# 3. the direct fixed-point iteration
@pytest.mark.parametrize("name", ["S400", "S310"])
def test_agreement_with_the_exact_iteration(fr, renderer, name):
    """The recorded exact iteration counts of tests/golden/deepx_ship_exact.npz (256 samples of the 128 x 96 frame).  The
    restatement alone agrees on 256 of 256 on both views (measured on the CPU, asserted in test_deepx_ship_bla_host.py); the
    bar is that less the 25-pixel margin of the Mandelbrot BLA tests."""
    g = SX.exact_golden()
    _, _, it = _render(fr, renderer, V[name], 128, 96)
    ex = g[name]
    largest = np.unique(ex, return_counts=True)[1].max() / len(ex)
    agree = int((it[g["ys"], g["xs"]] == ex).sum())
    print(name, "largest exact class", largest, "agreement", agree, "of", len(ex))
    assert largest <= 0.60                                         # a collapsed frame cannot agree by chance
    assert agree >= 256 - 25


# 4. plain-mode lanes taking BLA steps: views both ship BLA paths can render
@pytest.mark.parametrize("name", ["A", "B"])
def test_plain_mode_bla_against_fr_render_deep_ship_bla(fr, renderer, name):
    """fr_render_deepx_ship + FR_FLAG_DEEPX_SHIP_BLA against fr_render_deep_ship + FR_FLAG_DEEP_SHIP_BLA at 128 x 96: the number
    of iter values that differ and the difference of the step counts are whatever the two restatements give on the CPU --
    the GPU must give the same.  Measured on the CPU: 0 differing iter values and equal counts on both views
    ([1209695, 33448, 906142], [1683896, 48794, 5137212])."""
    w, h = 128, 96
    v = S.VIEWS[name]
    it_x = _render(fr, renderer, SX.as_x_view(v), w, h)[2]
    steps_x = np.array(renderer.last_deepx_ship_steps(), np.int64)
    it_d = np.empty((h, w), np.int32)
    renderer.render_deep_ship(fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"]), w, h, fr.DeepView(v["cx"], v["cy"]),
                              iter=it_d, bla=True)
    steps_d = np.array(renderer.last_deep_ship_steps(), np.int64)
    sx, cx = XB.restate_ship_x_bla(SX.as_x_view(v), w, h)
    sd, cd = SB.restate_bla(v, w, h, 1)
    cpu = int((sx[0][0] != sd[0][0]).sum())
    gpu = int((it_x != it_d).sum())
    print(name, "iter values that differ: restatements", cpu, "GPU", gpu, "count differences", steps_x - steps_d,
          np.array(cx) - np.array(cd))
    assert gpu == cpu
    assert tuple(steps_x - steps_d) == tuple(np.array(cx, np.int64) - np.array(cd, np.int64))
    assert tuple(steps_x) == tuple(cx) and steps_x[1] > 0
    assert np.array_equal(it_x, sx[0][0])


# 5. the unflagged path
@pytest.mark.parametrize("name", ["S400", "S310"])
def test_agreement_with_the_unflagged_path(fr, renderer, name):
    """iter values equal to fr_render_deepx_ship's without the flag on the same context: at least the restatements' own
    number (12279 and 12241 of 12288, test_deepx_ship_bla_host.py) less 25."""
    it_bla = _render(fr, renderer, V[name], 128, 96)[2]
    it_off = _render(fr, renderer, V[name], 128, 96, bla=False)[2]
    own = int((_restated(name)[0][0][0] == _unflagged(name)[0][0]).sum())
    got = int((it_bla == it_off).sum())
    print(name, "equal iter: restatements", own, "GPU", got, "of", it_bla.size)
    assert own == EQUAL_TO_UNFLAGGED[name]
    assert got >= own - 25


# 6. edge cases at 64 x 48
@pytest.mark.parametrize("v", [V["TIP400"], dict(cx="-1.75", cy="0", zoom="1e-320", max_iter=500)], ids=["TIP400", "cy0"])
def test_real_axis_views_take_no_bla_step(fr, renderer, v):
    """Y = 0 on the whole orbit: every radius is 0, no probe passes, and the planes are the unflagged bytes"""
    got = _render(fr, renderer, v, 64, 48, 2, True)
    steps = tuple(renderer.last_deepx_ship_steps())
    assert steps[0] > 0 and steps[1:] == (0, 0)
    assert _same(got, _render(fr, renderer, v, 64, 48, 2, True, bla=False))


def test_the_sample_with_dc_zero(fr, renderer):
    """even W and H: the centre pixel's sample has dc = 0, its dz stays 0 and passes every probe with r > 0"""
    v = V["S400"]
    w, h = 64, 48
    it = _render(fr, renderer, v, w, h)[2]
    samples, counts = XB.restate_ship_x_bla(v, w, h, orbit=_orbit("S400"))
    assert np.array_equal(it, samples[0][0]) and tuple(renderer.last_deepx_ship_steps()) == tuple(counts)
    zm, ze = X.zoom_pair(v["zoom"])
    dc = SX.sample_dc_ship_x(w, h, zm, ze, 1, 0, rows=[h // 2])
    assert dc[0][w // 2] == 0.0 and dc[1][w // 2] == 0.0 and dc[2][w // 2] == X.X_ZERO


@pytest.mark.parametrize("max_iter", [2, 3, 5, 9, 17, 1025])
def test_short_orbits_and_power_of_two_lengths(fr, renderer, max_iter):
    """S400's orbit cut by max_iterations: N = max_iter.  N <= 2 has no table and takes single steps only; N - 1 a power of
    two has one entry at the top level, which covers the whole orbit from m = 1."""
    v = dict(V["S400"], max_iter=max_iter)
    w, h = 64, 48
    orbit = SX.orbit_of(v)
    assert len(orbit[1]) - 1 == max_iter
    tab = XB.table_of(v, w, h, orbit)
    samples, counts = XB.restate_ship_x_bla(v, w, h, orbit=orbit, table=tab)
    rgba, nu, it = _render(fr, renderer, v, w, h)
    assert np.array_equal(it, samples[0][0])
    assert np.abs(nu - S.smooth(samples[0][0], samples[0][1], max_iter)).max() <= NU_TOL
    assert tuple(renderer.last_deepx_ship_steps()) == tuple(counts)
    n = fr.lib().fr_deepx_ship_bla_table(renderer._ctx, None, None, None, 0)
    if max_iter == 2:
        assert tab == [] and counts[1] == 0
    else:
        assert len(tab) == (max_iter - 1).bit_length() - 1 and len(tab[-1]["rv"]) == 1 and counts[1] > 0
        assert n == (max_iter - 1) - 1


# 7. shards, layouts, memory kinds, the asynchronous form
def test_shards_layouts_memory_and_async(fr, renderer):
    import torch
    v = V["S400"]
    w, h = 203, 117
    ref = _render(fr, renderer, v, w, h, 2, True)
    ref_rgba, ref_nu, ref_it = ref
    ref_steps = renderer.last_deepx_ship_steps()
    assert ref_steps.bla > 0 and len(np.unique(ref_it)) > 5
    for nparts in (1, 3, 8):
        rgba = np.zeros_like(ref_rgba); nu = np.zeros_like(ref_nu); it = np.full_like(ref_it, -7)
        tot = np.zeros(3, np.int64)
        for part in range(nparts):
            sh = fr.Shard(part, nparts)
            g = sh.global_rows(h)
            a, n, i = _render(fr, renderer, v, w, h, 2, True, shard=sh)
            rgba[g], nu[g], it[g] = a, n, i
            if sh.rows(h):
                tot += np.array(renderer.last_deepx_ship_steps())
        assert _same((rgba, nu, it), ref), nparts
        assert tuple(tot) == tuple(ref_steps), nparts                   # the counts of a call cover its own pixels
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
            renderer.render_deepx_ship(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it, bla=True)
        else:
            renderer.render_deepx_ship(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it,
                                       stream=s.cuda_stream, sync=False, bla=True)
            s.synchronize()
            renderer.check()
        assert renderer.last_deepx_ship_steps() == ref_steps, sync
        assert _same((d_rgba.cpu().numpy(), d_nu.cpu().numpy(), d_it.cpu().numpy()), ref), sync
    # FR_LAYOUT_FRAME: each part writes its rows in place into whole-frame device planes
    L = fr.lib()
    p = st.to_params(fr.FractalType.BurningShip, fr.Precision.F64, True)
    p.flags |= fr.FR_FLAG_DEEPX_SHIP_BLA
    cv = view.to_cx()
    d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
    d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
    d_it = torch.full((h, w), -7, dtype=torch.int32, device=dev)
    o = fr._capi.fr_output(d_rgba.data_ptr(), d_nu.data_ptr(), d_it.data_ptr(), fr._capi.FR_MEM_DEVICE, fr._capi.FR_LAYOUT_FRAME)
    torch.cuda.synchronize()
    for part in range(3):
        sh = fr._capi.fr_shard(part, 3, 16)
        assert L.fr_render_deepx_ship(renderer._ctx, C.byref(p), C.byref(cv), w, h, C.byref(sh), C.byref(o)) == 0
    assert _same((d_rgba.cpu().numpy(), d_nu.cpu().numpy(), d_it.cpu().numpy()), ref)


# 8. the caches of one context
def test_caches_across_paths(fr):
    """S400 with and without the flag, a zoom change at S400's centre (the table is rebuilt, the orbit kept), S310,
    fr_render_deepx with its BLA and fr_render_deep_ship with its BLA on one context, interleaved: every frame equals the
    same frame rendered alone, and each path's counts stay its own"""
    w, h = 96, 72
    s2 = dict(V["S400"], zoom="2e-400")
    xd = X.views()["T300"]
    sa = S.SHIP_A

    def shipx(r, v, flag):
        out = _render(fr, r, v, w, h, 1, True, bla=flag)
        return out + ((tuple(r.last_deepx_ship_steps()),) if flag else ())

    def deepx_bla(r):
        out = (np.empty((h, w, 4), np.float32), np.empty((h, w), np.float64), np.empty((h, w), np.int32))
        r.render_deep(fr.FractalState(max_iterations=xd["max_iter"]), w, h, fr.DeepView(xd["cx"], xd["cy"], zoom=xd["zoom"]),
                      post_chain=True, rgba=out[0], nu=out[1], iter=out[2], xbla=True)
        return out + (tuple(r.last_deepx_steps()),)

    def ship_bla(r):
        out = (np.empty((h, w, 4), np.float32), np.empty((h, w), np.float64), np.empty((h, w), np.int32))
        r.render_deep_ship(fr.FractalState(zoom=sa["zoom"], max_iterations=sa["max_iter"]), w, h, fr.DeepView(sa["cx"], sa["cy"]),
                           post_chain=True, rgba=out[0], nu=out[1], iter=out[2], bla=True)
        return out + (tuple(r.last_deep_ship_steps()),)

    jobs = {"Sb": lambda r: shipx(r, V["S400"], True), "Sp": lambda r: shipx(r, V["S400"], False),
            "S2b": lambda r: shipx(r, s2, True), "Tb": lambda r: shipx(r, V["S310"], True), "Xb": deepx_bla, "Hb": ship_bla}
    alone = {}
    for key, fn in jobs.items():
        with fr.Renderer(0) as r:
            alone[key] = fn(r)
    assert alone["Sb"][3] != alone["S2b"][3] and alone["Sb"][3][1] > 0
    with fr.Renderer(0) as r:
        for key in ("Sb", "Sp", "Sb", "S2b", "Sb", "Xb", "Tb", "Sp", "Hb", "S2b", "Xb", "Tb", "Hb", "Sb"):
            got = jobs[key](r)
            for g, want in zip(got, alone[key]):
                assert np.array_equal(np.asarray(g).view(np.uint8), np.asarray(want).view(np.uint8)), key
        # each path's counts are still those of its own last call
        assert tuple(r.last_deepx_steps()) == alone["Xb"][3] and tuple(r.last_deep_ship_steps()) == alone["Hb"][3]
        assert tuple(r.last_deepx_ship_steps()) == alone["Sb"][3]


# 9. the interface
def test_interface(fr):
    K = fr._capi
    U = K.FR_ERR_UNSUPPORTED
    L = fr.lib()
    NEW = fr.FR_FLAG_DEEPX_SHIP_BLA
    assert NEW == 0x10
    w, h = 64, 48
    v = V["S400"]
    with fr.Renderer(0) as r:
        with pytest.raises(fr.FractalRendererError):
            r.last_deepx_ship_steps()
        _render(fr, r, v, w, h, bla=False)                          # without the flag: still no counts
        with pytest.raises(fr.FractalRendererError):
            r.last_deepx_ship_steps()

        def planes():
            return [np.empty((h, w, 4), np.float32), np.empty((h, w), np.float64), np.empty((h, w), np.int32)]

        def out_of(pl):
            return K.fr_output(pl[0].ctypes.data, pl[1].ctypes.data, pl[2].ctypes.data, K.FR_MEM_HOST, 0)

        # the other entry points ignore 0x10: the bytes they write without it, and no counts of any kind
        a, xa, sa = R.VIEW_A, X.views()["T300"], S.SHIP_A
        mandel, ship, f64 = fr.FractalType.Mandelbrot, fr.FractalType.BurningShip, fr.Precision.F64
        calls = {
            "fr_render": (fr.FractalState(max_iterations=200), mandel,
                          lambda p, o: L.fr_render(r._ctx, C.byref(p), w, h, C.byref(o))),
            "fr_render_deep": (fr.FractalState(zoom=a["zoom"], max_iterations=a["max_iter"]), mandel,
                               lambda p, o: L.fr_render_deep(r._ctx, C.byref(p), C.byref(fr.DeepView(a["cx"], a["cy"]).to_c()),
                                                             w, h, None, C.byref(o))),
            "fr_render_deepx": (fr.FractalState(max_iterations=xa["max_iter"]), mandel,
                                lambda p, o: L.fr_render_deepx(r._ctx, C.byref(p), C.byref(
                                    fr.DeepView(xa["cx"], xa["cy"], zoom=xa["zoom"]).to_cx()), w, h, None, C.byref(o))),
            "fr_render_deep_ship": (fr.FractalState(zoom=sa["zoom"], max_iterations=sa["max_iter"]), ship,
                                    lambda p, o: L.fr_render_deep_ship(r._ctx, C.byref(p), C.byref(
                                        fr.DeepView(sa["cx"], sa["cy"]).to_c()), w, h, None, C.byref(o))),
        }
        for name, (st, ftype, call) in calls.items():
            got, want = planes(), planes()
            for flags, pl in ((NEW, got), (0, want)):
                p = st.to_params(ftype, f64, False)
                p.flags |= flags
                assert call(p, out_of(pl)) == 0, name
            assert _same(got, want), name
        for counts in (r.last_deep_steps, r.last_deepx_steps, r.last_deep_ship_steps, r.last_deepx_ship_steps):
            with pytest.raises(fr.FractalRendererError):
                counts()
        # the three old flags stay unsupported here, alone or with the new one
        it = np.empty((8, 8), np.int32)
        o = K.fr_output(None, None, it.ctypes.data, K.FR_MEM_HOST, 0)
        cx = fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"]).to_cx()
        for old in (fr.FR_FLAG_DEEP_BLA, fr.FR_FLAG_DEEPX_BLA, fr.FR_FLAG_DEEP_SHIP_BLA):
            for flags in (old, old | NEW):
                p = fr.FractalState(max_iterations=64).to_params(ship, f64, False)
                p.flags |= flags
                assert L.fr_render_deepx_ship(r._ctx, C.byref(p), C.byref(cx), 8, 8, None, C.byref(o)) == U, flags
        with pytest.raises(fr.FractalRendererError):
            r.last_deepx_ship_steps()
        p = fr.FractalState(max_iterations=64).to_params(ship, f64, False)
        p.flags |= NEW
        assert L.fr_render_deepx_ship(r._ctx, C.byref(p), C.byref(cx), 8, 8, None, C.byref(o)) == 0
        assert r.last_deepx_ship_steps().plain > 0
        for other in (r.last_deep_steps, r.last_deepx_steps, r.last_deep_ship_steps):
            with pytest.raises(fr.FractalRendererError):
                other()


# 10. a ship sequence with the flag
@pytest.mark.parametrize("keyframes", [False, True], ids=["mode0", "mode1"])
def test_ship_sequence_with_the_flag(fr, keyframes):
    """5 frames at 96 x 72 from 4e-400 to 2.5e-401 into S400's centre: four octaves, so every frame lies on the keyframe grid
    and has a decimal zoom string.  Each frame equals fr_render_deepx_ship with the flag at that string and the sequence's
    F, and the counts of the context are those of that render."""
    w, h = 96, 72
    v = V["S400"]
    zooms = ["4e-400", "2e-400", "1e-400", "5e-401", "2.5e-401"]
    st = fr.FractalState(max_iterations=v["max_iter"])
    frames, counts = [], []
    with fr.Renderer(0) as r:
        with fr.DeepZoomSequence(r, st, v["cx"], v["cy"], zooms[0], zooms[-1], 5, w, h, keyframes=keyframes, formula="ship",
                                 bla=True, post_chain=True) as seq:
            F = seq.plan(0).frac_bits
            for f in range(5):
                pl = seq.plan(f)
                assert (pl.zoom_mant, pl.zoom_exp2) == X.zoom_pair(zooms[f]) and not pl.resampled
                out = (np.empty((h, w, 4), np.float32), np.empty((h, w), np.float64), np.empty((h, w), np.int32))
                seq.render(f, rgba=out[0], nu=out[1], iter=out[2])
                frames.append(out)
                counts.append(tuple(r.last_deepx_ship_steps()))
    with fr.Renderer(0) as r:
        for f in range(5):
            want = _render(fr, r, dict(v, zoom=zooms[f], frac_bits=F), w, h, 1, True)
            assert _same(frames[f], want), f
            assert counts[f] == tuple(r.last_deepx_ship_steps()) and counts[f][1] > 0, f
    assert len(set(counts)) == 5
