"""Extended views with bilinear approximation on the GPU (fr_render_deepx with FR_FLAG_DEEPX_BLA): the planes and the step
counts against the numpy restatement (tests/deepx_bla_ref.py), the device-built table against numpy's bit for bit, the
direct fixed-point iteration, fr_render_deep's fp64 BLA where both can render a view, the unflagged path, edge cases,
shards, layouts, memory kinds, the asynchronous form and the caches of one context."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_bla_ref as BR
import deep_ref as R
import deepx_bla_ref as XB
import deepx_ref as X
from test_deep_bla_gpu import _render as _render_fp64_bla, _restated as _restated_fp64_bla
from test_deep_gpu import NU_TOL, RGB_TOL, _few
from test_deepx_gpu import E_ROWS, _check_exact, _expected_rgba, _render_x, _restated as _restated_unflagged, _xview

pytestmark = pytest.mark.gpu

W, H = 256, 192
V = X.views()
SHALLOW = dict(R.VIEWS, C=BR.VIEW_C)


def _render(fr, r, v, aa=1, post=False, shard=None, w=W, h=H, **kw):
    return _render_x(fr, r, v, aa, post, shard, w, h, xbla=True, **kw)


@functools.lru_cache(maxsize=None)
def _orbit(name):
    return X.orbit_of(V[name])


def _restated(name, aa=1):
    return _restated_once(name, aa)


@functools.lru_cache(maxsize=None)
def _restated_once(name, aa):
    """computed once, shared by every test, never changed"""
    if name in V:
        return XB.restate_x_bla(V[name], W, H, aa, orbit=_orbit(name))
    return XB.restate_x_bla(_xview(name) if name != "C" else _as_x(BR.VIEW_C), W, H, aa)


def _as_x(v):
    return dict(cx=v["cx"], cy=v["cy"], zoom=repr(v["zoom"]), max_iter=v["max_iter"])


def _check_planes(oracle, v, got, samples, aa, post):
    rgba, nu, it = got
    r_it, r_r2 = samples[0]
    ndiff = int((it != r_it).sum())
    dnu = float(np.abs(nu - R.smooth(r_it, r_r2, v["max_iter"])).max())
    bad = np.abs(rgba[..., :3] - _expected_rgba(oracle, v, samples, aa, post)).max(axis=2) > RGB_TOL
    print("iter differences", ndiff, "max |nu - restated|", dnu, "rgb outside tolerance", int(bad.sum()), "of", it.size)
    assert ndiff == 0
    assert dnu <= NU_TOL
    assert np.all(rgba[..., 3] == 1.0)
    assert _few(bad, it.size), int(bad.sum())


# 1. planes and counts equal the restatement
@pytest.mark.parametrize("name,aa,post", [("D", 1, False), ("D", 2, True), ("E", 1, True)] +
                         [(n, 1, False) for n in ("T110", "T130", "T260", "T280", "T300", "T320")])
def test_planes_and_counts_match_the_restatement(fr, renderer, oracle, name, aa, post):
    v = V[name]
    got = _render(fr, renderer, v, aa, post)
    steps = tuple(renderer.last_deepx_steps())
    samples, counts = _restated(name, aa)
    print(name, "counts", steps, "restated", tuple(counts))
    if name == "E":                                                # the band of rows test_deepx_gpu restates
        got = tuple(p[E_ROWS] for p in got)
        samples = [(a[E_ROWS], b[E_ROWS]) for a, b in samples]
    _check_planes(oracle, v, got, samples, aa, post)
    # every table radius and every level choice of the kernel, summed over the whole frame: equal, not close
    assert steps == tuple(counts)
    assert counts[1] > 0 and counts[2] > counts[0]


# 2. the device table, through its sqrt and division included
@pytest.mark.parametrize("name", ["D", "T300"])
def test_device_table_equals_numpy_bit_for_bit(fr, renderer, name):
    v = V[name]
    _render(fr, renderer, v)
    tab = XB.table_of(v, W, H, _orbit(name))
    n = sum(len(T["rv"]) for T in tab)
    r = np.empty(n, np.dtype([("v", np.float32), ("e", np.int32)]))
    ab = np.empty((n, 4), np.float64)
    abe = np.empty((n, 2), np.int32)
    got = fr.lib().fr_deepx_bla_table(renderer._ctx, r.ctypes.data, ab.ctypes.data, abe.ctypes.data, n)
    assert got == n
    want_rv = np.concatenate([T["rv"] for T in tab]).astype(np.float32)
    want_re = np.concatenate([T["re"] for T in tab]).astype(np.int32)
    want_ab = np.concatenate([np.stack([T["ax"], T["ay"], T["bx"], T["by"]], axis=1) for T in tab])
    want_abe = np.concatenate([np.stack([T["ea"], T["eb"]], axis=1) for T in tab]).astype(np.int32)
    assert np.array_equal(r["v"].view(np.uint32), want_rv.view(np.uint32)) and np.array_equal(r["e"], want_re)
    assert np.array_equal(ab.view(np.uint64), want_ab.view(np.uint64))
    assert np.array_equal(abe, want_abe)
    assert (r["v"] > 0).all()


# 3. the direct fixed-point iteration: the bar of the host test (0.99, largest share 0.60)
@pytest.mark.parametrize("name", ["D", "E"])
def test_agreement_with_the_exact_iteration(fr, renderer, name):
    _, _, it = _render(fr, renderer, V[name])
    _check_exact(name, it)


# 4. plain-mode lanes taking BLA steps: views both BLA paths can render
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_plain_mode_bla_against_fr_render_deep_bla(fr, renderer, name):
    """fr_render_deepx + FR_FLAG_DEEPX_BLA against fr_render_deep + FR_FLAG_DEEP_BLA: the number of iter values that differ
    and the difference of the step counts are whatever the two restatements give on the CPU -- the GPU must give the same.
    Measured on the CPU: 0 differing iter values and equal counts on A, B and C ([6726863, 173982, 5549050],
    [6736528, 220328, 33450138], [8007818, 3362807, 157366052])."""
    v = SHALLOW[name]
    it_x = _render(fr, renderer, _as_x(v))[2]
    steps_x = np.array(renderer.last_deepx_steps(), np.int64)
    it_d = _render_fp64_bla(fr, renderer, v)[2]
    steps_d = np.array(renderer.last_deep_steps(), np.int64)
    sx, cx = _restated(name)
    sd, cd = _restated_fp64_bla(name, 1)
    cpu = int((sx[0][0] != sd[0][0]).sum())
    gpu = int((it_x != it_d).sum())
    print(name, "iter values that differ: restatements", cpu, "GPU", gpu, "count differences", steps_x - steps_d,
          np.array(cx) - np.array(cd))
    assert gpu == cpu
    assert tuple(steps_x - steps_d) == tuple(np.array(cx, np.int64) - np.array(cd, np.int64))
    assert tuple(steps_x) == tuple(cx) and steps_x[1] > 0
    assert np.array_equal(it_x, sx[0][0])


# 5. the unflagged path
@pytest.mark.parametrize("name", ["D", "T320"])
def test_agreement_with_the_unflagged_path(fr, renderer, name):
    """Share of pixels whose iter equals fr_render_deepx's without the flag on the same context: at least the restatements'
    own share less 25 pixels (the margin of test_deep_bla_gpu.test_agreement_with_the_plain_path).  The restatements give
    1.0 on both views (49152 of 49152 pixels)."""
    v = V[name]
    it_bla = _render(fr, renderer, v)[2]
    it_off = _render_x(fr, renderer, v)[2]
    own = int((_restated(name)[0][0][0] == _restated_unflagged(name, 1)[0][0][0]).sum())
    got = int((it_bla == it_off).sum())
    print(name, "equal iter: restatements", own, "GPU", got, "of", W * H)
    assert got >= own - 25


# 6. edge cases
def test_the_sample_with_dc_zero(fr, renderer):
    """even W and H: the centre pixel's sample has dc = 0, its dz stays 0 and passes every probe"""
    v = V["T320"]
    it = _render(fr, renderer, v)[2]
    r_it = _restated("T320")[0][0][0]
    assert it[H // 2, W // 2] == r_it[H // 2, W // 2]
    zm, ze = X.zoom_pair(v["zoom"])
    dc = X.sample_dc_x(W, H, zm, ze, 1, 0, rows=[H // 2])
    assert dc[0][W // 2] == 0.0 and dc[1][W // 2] == 0.0 and dc[2][W // 2] == X.X_ZERO


def test_centre_zero_takes_no_bla_step(fr, renderer):
    v = dict(cx="0", cy="0", zoom="1e-320", max_iter=500)
    a, n, i = _render(fr, renderer, v, 2, True)
    assert tuple(renderer.last_deepx_steps())[1:] == (0, 0)
    a0, n0, i0 = _render_x(fr, renderer, v, 2, True)
    assert np.array_equal(a.view(np.uint8), a0.view(np.uint8)) and np.array_equal(n.view(np.uint8), n0.view(np.uint8)) \
        and np.array_equal(i, i0)


@pytest.mark.parametrize("max_iter", [700, 1025, 2500])
def test_short_iteration_budgets_and_power_of_two_orbits(fr, renderer, max_iter):
    """D's orbit (N = 3257 at its own budget) cut by max_iterations: N = max_iter, never reached by a rebase-free sample
    before the budget ends; 1025: N - 1 = 1024, one entry at the top level.  64 x 48 frames."""
    v = dict(V["D"], max_iter=max_iter)
    w, h = 64, 48
    orbit = X.orbit_of(v)
    assert len(orbit[1]) - 1 == max_iter
    samples, counts = XB.restate_x_bla(v, w, h, orbit=orbit)
    rgba, nu, it = _render(fr, renderer, v, w=w, h=h)
    assert np.array_equal(it, samples[0][0])
    assert np.abs(nu - R.smooth(samples[0][0], samples[0][1], max_iter)).max() <= NU_TOL
    assert tuple(renderer.last_deepx_steps()) == tuple(counts) and counts[1] > 0
    if max_iter == 1025:
        tab = XB.table_of(v, w, h, orbit)
        assert len(tab) == 10 and len(tab[-1]["rv"]) == 1


# 7. shards, layouts, memory kinds, the asynchronous form
def test_shards_layouts_memory_and_async(fr, renderer):
    import torch
    v = V["D"]
    w, h = 203, 117
    ref_rgba, ref_nu, ref_it = _render(fr, renderer, v, 2, True, w=w, h=h)
    ref_steps = renderer.last_deepx_steps()
    assert ref_steps.bla > 0 and len(np.unique(ref_it)) > 5
    for nparts in (1, 3, 8):
        rgba = np.zeros_like(ref_rgba); nu = np.zeros_like(ref_nu); it = np.full_like(ref_it, -7)
        tot = np.zeros(3, np.int64)
        for part in range(nparts):
            sh = fr.Shard(part, nparts)
            g = sh.global_rows(h)
            a, n, i = _render(fr, renderer, v, 2, True, shard=sh, w=w, h=h)
            rgba[g], nu[g], it[g] = a, n, i
            if sh.rows(h):
                tot += np.array(renderer.last_deepx_steps())
        assert np.array_equal(rgba, ref_rgba) and np.array_equal(nu.view(np.uint64), ref_nu.view(np.uint64)) \
            and np.array_equal(it, ref_it), nparts
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
            renderer.render_deep(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it, xbla=True)
        else:
            renderer.render_deep(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it,
                                 stream=s.cuda_stream, sync=False, xbla=True)
            s.synchronize()
            renderer.check()
        assert renderer.last_deepx_steps() == ref_steps, sync
        assert np.array_equal(d_rgba.cpu().numpy(), ref_rgba) and np.array_equal(d_it.cpu().numpy(), ref_it)
        assert np.array_equal(d_nu.cpu().numpy().view(np.uint64), ref_nu.view(np.uint64)), sync
    # FR_LAYOUT_FRAME: each part writes its rows in place into whole-frame device planes
    L = fr.lib()
    p = st.to_params(fr.FractalType.Mandelbrot, fr.Precision.F64, True)
    p.flags |= fr.FR_FLAG_DEEPX_BLA
    cv = view.to_cx()
    d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
    d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
    d_it = torch.full((h, w), -7, dtype=torch.int32, device=dev)
    o = fr._capi.fr_output(d_rgba.data_ptr(), d_nu.data_ptr(), d_it.data_ptr(), fr._capi.FR_MEM_DEVICE, fr._capi.FR_LAYOUT_FRAME)
    torch.cuda.synchronize()
    for part in range(3):
        sh = fr._capi.fr_shard(part, 3, 16)
        assert L.fr_render_deepx(renderer._ctx, C.byref(p), C.byref(cv), w, h, C.byref(sh), C.byref(o)) == 0
    assert np.array_equal(d_rgba.cpu().numpy(), ref_rgba) and np.array_equal(d_it.cpu().numpy(), ref_it)
    assert np.array_equal(d_nu.cpu().numpy().view(np.uint64), ref_nu.view(np.uint64))


# 8. the caches of one context
def test_caches_across_paths(fr):
    """D with and without the flag, a zoom change at D's centre (the table is rebuilt, the orbit kept), T300,
    fr_render_deep with its BLA on B and a Phoenix frame on one context, interleaved: every frame equals the same frame
    rendered alone"""
    W2, H2 = 160, 120
    d2 = dict(V["D"], zoom="2e-400")

    def deepx(r, v, flag):
        out = _render_x(fr, r, v, 1, True, w=W2, h=H2, xbla=flag)
        return out + ((tuple(r.last_deepx_steps()),) if flag else ())

    def deep_bla(r):
        out = _render_fp64_bla(fr, r, R.VIEW_B, 1, True, w=W2, h=H2)
        return out + (tuple(r.last_deep_steps()),)

    def phoenix(r):
        rgba = np.empty((H2, W2, 4), np.float32)
        it = np.empty((H2, W2), np.int32)
        r.render_phoenix(fr.FractalState(max_iterations=300), W2, H2, precision=fr.Precision.F64, rgba=rgba, iter=it)
        return rgba, it

    jobs = {"Db": lambda r: deepx(r, V["D"], True), "Dp": lambda r: deepx(r, V["D"], False),
            "D2b": lambda r: deepx(r, d2, True), "Tb": lambda r: deepx(r, V["T300"], True), "Bb": deep_bla, "ph": phoenix}
    alone = {}
    for key, fn in jobs.items():
        with fr.Renderer(0) as r:
            alone[key] = fn(r)
    assert alone["Db"][3] != alone["D2b"][3]
    with fr.Renderer(0) as r:
        for key in ("Db", "Dp", "Db", "D2b", "Db", "Bb", "Tb", "Dp", "ph", "D2b", "Bb", "Tb", "Db"):
            got = jobs[key](r)
            for g, want in zip(got, alone[key]):
                assert np.array_equal(np.asarray(g).view(np.uint8), np.asarray(want).view(np.uint8)), key


# 9. the interface
def test_interface(fr):
    U = fr._capi.FR_ERR_UNSUPPORTED
    L = fr.lib()
    v = V["D"]
    with fr.Renderer(0) as r:
        with pytest.raises(fr.FractalRendererError):
            r.last_deepx_steps()
        _render_x(fr, r, v, w=64, h=48)                             # without the flag: still no counts
        with pytest.raises(fr.FractalRendererError):
            r.last_deepx_steps()
        # fr_render_deep ignores 0x4: the bytes of the plain render, no counts of either kind
        a = R.VIEW_A
        planes = [np.empty((48, 64, 4), np.float32), np.empty((48, 64), np.float64), np.empty((48, 64), np.int32)]
        want = [np.empty_like(p) for p in planes]
        st = fr.FractalState(zoom=a["zoom"], max_iterations=a["max_iter"])
        cv = fr.DeepView(a["cx"], a["cy"]).to_c()
        for flags, out in ((fr.FR_FLAG_DEEPX_BLA, planes), (0, want)):
            p = st.to_params(fr.FractalType.Mandelbrot, fr.Precision.F64, False)
            p.flags |= flags
            o = fr._capi.fr_output(out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, fr._capi.FR_MEM_HOST, 0)
            assert L.fr_render_deep(r._ctx, C.byref(p), C.byref(cv), 64, 48, None, C.byref(o)) == 0
        for g, w_ in zip(planes, want):
            assert np.array_equal(g.view(np.uint8), w_.view(np.uint8))
        with pytest.raises(fr.FractalRendererError):
            r.last_deepx_steps()
        with pytest.raises(fr.FractalRendererError):
            r.last_deep_steps()
        # 0x2 on fr_render_deepx stays unsupported, with or without 0x4
        it = np.empty((8, 8), np.int32)
        o = fr._capi.fr_output(None, None, it.ctypes.data, fr._capi.FR_MEM_HOST, 0)
        cx = fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"]).to_cx()
        for flags, want_st in ((fr.FR_FLAG_DEEP_BLA, U), (fr.FR_FLAG_DEEP_BLA | fr.FR_FLAG_DEEPX_BLA, U), (fr.FR_FLAG_DEEPX_BLA, 0)):
            p = fr.FractalState(max_iterations=64).to_params(fr.FractalType.Mandelbrot, fr.Precision.F64, False)
            p.flags |= flags
            assert L.fr_render_deepx(r._ctx, C.byref(p), C.byref(cx), 8, 8, None, C.byref(o)) == want_st, flags
        assert r.last_deepx_steps().plain > 0
        with pytest.raises(fr.FractalRendererError):
            _render_x(fr, r, v, w=8, h=8, bla=True, xbla=True)
        with pytest.raises(ValueError):
            r.render_deep(st, 8, 8, fr.DeepView(a["cx"], a["cy"]), iter=it, xbla=True)
