"""Deep Julia views with bilinear approximation on the GPU (fr_render_deep_julia with FR_FLAG_DEEP_JULIA_BLA, fr_render_deepx_julia
with FR_FLAG_DEEPX_JULIA_BLA): the planes and the step counts against the numpy restatement (tests/deep_julia_bla_ref.py), both
device-built tables against numpy's bit for bit, the unflagged path and the exact iteration, the plain-mode lanes of the
extended kernel against the fp64 kernel, edge cases, and the render paths and caches of one context.

iter and the counts are compared for equality.  nu and rgba follow from (iter, r2) through the colour stage of the unflagged
kernels; as in the other BLA tests they are compared with numpy's logarithm to NU_TOL / RGB_TOL, and byte for byte with the
unflagged render wherever no BLA step was taken."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_julia_bla_ref as JB
import deep_julia_ref as J
import deep_ship_ref as S
from test_deep_julia_bla_host import EQUAL_TO_UNFLAGGED, EXACT_AGREEMENT

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4
NU_TOL = 1e-9
W, H = JB.BW, JB.BH

FRAMES = {                              # case: (view, extended, W, H, aa, post)
    "RABBIT30": ("RABBIT30", False, W, H, 1, False),
    "DENDRITE100": ("DENDRITE100", False, W, H, 1, False),
    "PRECRIT60": ("PRECRIT60", False, W, H, 1, False),
    "RABBIT30-aa2-post": ("RABBIT30", False, 64, 48, 2, True),
    "DENDRITE400-x": ("DENDRITE400", True, W, H, 1, False),
    "PRECRIT60-x": ("PRECRIT60", True, W, H, 1, False),
    "PRECRIT60-x-aa2-post": ("PRECRIT60", True, 64, 48, 2, True),
}


def _few(bad, n):
    return int(bad.sum()) <= max(2, int(0.001 * n))


def _same(got, want):
    return all(np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)) for g, w in zip(got, want))


def _state(fr, v, aa=1, extended=False):
    # the extended entry point does not read state.zoom: give it one no view of the tests has
    return fr.FractalState(zoom=2.5 if extended else v["zoom"], max_iterations=v["max_iter"], antialiasing_samples=aa,
                           julia_c_real=v["c"][0], julia_c_imag=v["c"][1])


def _view(fr, v, extended):
    return fr.DeepView(v["cx"], v["cy"], frac_bits=v.get("frac_bits", 0), zoom=v["zoom_s"] if extended else None)


def _render(fr, r, v, w, h, aa=1, post=False, extended=False, bla=True, shard=None):
    rows = shard.rows(h) if shard else h
    rgba = np.empty((rows, w, 4), np.float32)
    nu = np.empty((rows, w), np.float64)
    it = np.empty((rows, w), np.int32)
    r.render_deep_julia(_state(fr, v, aa, extended), w, h, _view(fr, v, extended), post_chain=post, rgba=rgba, nu=nu, iter=it,
                        shard=shard, bla=bla)
    return rgba, nu, it


def _steps(r, extended):
    return tuple(r.last_deepx_julia_steps() if extended else r.last_deep_julia_steps())


def _restate(v, extended, w, h, aa=1, **kw):
    return (JB.restate_x_bla if extended else JB.restate_bla)(v, w, h, aa, **kw)


@functools.lru_cache(maxsize=None)
def _restated(case):
    """computed once per frame, shared, never changed: the samples, the three counts, the per-orbit BLA steps"""
    name, extended, w, h, aa, _ = FRAMES[case]
    return (JB.restated_x_bla if extended else JB.restated_bla)(name, aa, w, h)


def _expected_rgb(oracle, v, samples, aa, post):
    p = oracle.OracleParams(fractal=1, max_iterations=v["max_iter"], aa=aa, post_chain=0)
    h, w = samples[0][0].shape
    acc = np.zeros((h, w, 3), np.float32)
    for s_it, s_r2 in samples:
        acc = acc + oracle.colorize(p, J.smooth(s_it, s_r2, v["max_iter"]))[..., :3]
    if aa > 1:
        acc = acc / np.float32(aa * aa)
    if post:
        acc = np.array([oracle.post_chain(c, julia_floors=1) for c in acc.reshape(-1, 3)], np.float32).reshape(h, w, 3)
    return acc


def _check_planes(oracle, v, got, samples, aa, post):
    rgba, nu, it = got
    r_it, r_r2 = samples[0]
    ndiff = int((it != r_it).sum())
    dnu = float(np.abs(nu - J.smooth(r_it, r_r2, v["max_iter"])).max())
    bad = np.abs(rgba[..., :3] - _expected_rgb(oracle, v, samples, aa, post)).max(axis=2) > RGB_TOL
    print("iter differences", ndiff, "max |nu - restated|", dnu, "rgb outside tolerance", int(bad.sum()), "of", it.size)
    assert ndiff == 0
    assert dnu <= NU_TOL
    assert np.all(rgba[..., 3] == 1.0)
    assert _few(bad, it.size), int(bad.sum())


# 1. planes and counts equal the restatement
@pytest.mark.parametrize("case", list(FRAMES))
def test_planes_and_counts_match_the_restatement(fr, renderer, oracle, case):
    """Fails without the feature: the flag is ignored today and the counters do not exist."""
    name, extended, w, h, aa, post = FRAMES[case]
    v = JB.view(name)
    got = _render(fr, renderer, v, w, h, aa, post, extended)
    steps = _steps(renderer, extended)
    samples, counts, stats = _restated(case)
    print(case, "counts", steps, "restated", tuple(counts), stats)
    _check_planes(oracle, v, got, samples, aa, post)
    # every table radius and every level choice of the kernel, on both orbits, summed over the whole frame: equal, not close
    assert steps == tuple(counts)
    assert counts[1] > 0 and counts[2] > counts[0]
    if name == "PRECRIT60":
        assert stats["bla_q"] > 0 and stats["bla_p"] > 0


# 2. both device tables and their order
def test_device_tables_equal_numpy_bit_for_bit(fr, renderer):
    v = JB.view("RABBIT30")
    _render(fr, renderer, v, 64, 48)
    P, Q = JB.orbits("RABBIT30")
    tabs = JB.bla_tables(P, Q)
    want_r, want_a = JB.flat(tabs)
    n = len(want_r)
    assert n == JB.entries(len(Q) - 1) + JB.entries(len(P) - 1) and len(tabs[0]) > 0 and len(tabs[1]) > 0
    r = np.empty(n, np.float64)
    a = np.empty((n, 2), np.float64)
    L = fr.lib()
    assert L.fr_deep_julia_bla_table(renderer._ctx, None, None, 0) == n
    assert L.fr_deep_julia_bla_table(renderer._ctx, r.ctypes.data, a.ctypes.data, n) == n
    assert np.array_equal(r.view(np.uint64), want_r.view(np.uint64))
    assert np.array_equal(a.view(np.uint64), np.ascontiguousarray(want_a).view(np.uint64))
    assert (r > 0).sum() > n // 2


def test_extended_device_tables_equal_numpy_bit_for_bit(fr, renderer):
    v = JB.view("DENDRITE400")
    _render(fr, renderer, v, 48, 36, extended=True)
    Px, Qx = JB.orbits_x("DENDRITE400")
    tabs = JB.bla_tables_x(Px, Qx)
    want_rv, want_re, want_a, want_ea = JB.flat_x(tabs)
    n = len(want_rv)
    assert n == JB.entries(len(Qx[1]) - 1) + JB.entries(len(Px[1]) - 1) and len(tabs[0]) > 0 and len(tabs[1]) > 0
    r = np.empty(n, np.dtype([("v", np.float32), ("e", np.int32)]))
    a = np.empty((n, 2), np.float64)
    ae = np.empty(n, np.int32)
    L = fr.lib()
    assert L.fr_deepx_julia_bla_table(renderer._ctx, None, None, None, 0) == n
    assert L.fr_deepx_julia_bla_table(renderer._ctx, r.ctypes.data, a.ctypes.data, ae.ctypes.data, n) == n
    assert np.array_equal(r["v"].view(np.uint32), want_rv.view(np.uint32)) and np.array_equal(r["e"], want_re)
    assert np.array_equal(a.view(np.uint64), np.ascontiguousarray(want_a).view(np.uint64))
    assert np.array_equal(ae, want_ea)
    assert (r["v"] > 0).sum() > n // 2


# 3. the unflagged path and the exact iteration
@pytest.mark.parametrize("name,extended", [("RABBIT30", False), ("DENDRITE100", False), ("PRECRIT60", False), ("DENDRITE400", True),
                                           ("PRECRIT60", True)])
def test_agreement_with_the_unflagged_path(fr, renderer, name, extended):
    """iter values equal to the same entry point's without the flag on the same context: at least the restatements' own
    number (test_deep_julia_bla_host.py) less 25"""
    v = JB.view(name)
    it_bla = _render(fr, renderer, v, W, H, extended=extended)[2]
    it_off = _render(fr, renderer, v, W, H, extended=extended, bla=False)[2]
    own = EQUAL_TO_UNFLAGGED[name + ("-x" if extended else "")]
    got = int((it_bla == it_off).sum())
    print(name, extended, "equal iter: restatements", own, "GPU", got, "of", it_bla.size)
    assert got >= own - 25


@pytest.mark.parametrize("name,extended", [("DENDRITE100", False), ("DENDRITE400", True)])
def test_agreement_with_the_exact_iteration(fr, renderer, name, extended):
    """the fixed-point samples of deep_julia_ref: the restatement's own agreement (test_deep_julia_bla_host.py) less 25.  The
    views are those whose largest exact class stays below 0.60 of the samples (RABBIT30's is 0.73)."""
    v = JB.view(name)
    w, h = (J.XW, J.XH) if extended else (W, H)
    it = _render(fr, renderer, v, w, h, extended=extended)[2]
    ex = J.exact_samples_x(name) if extended else J.exact_samples(name, w, h)
    ys, xs = J.random_pixels(w, h)
    largest = np.unique(ex, return_counts=True)[1].max() / len(ex)
    agree = int((it[ys, xs] == ex).sum())
    print(name, "largest exact class", largest, "agreement", agree, "of", len(ex))
    assert largest <= 0.60                                         # a collapsed frame cannot agree by chance
    assert agree >= EXACT_AGREEMENT[name] - 25


# 4. plain-mode lanes of the extended kernel
@pytest.mark.parametrize("name", ["RABBIT30", "DENDRITE100"])
def test_plain_mode_lanes_against_the_fp64_kernel(fr, renderer, name):
    """fr_render_deepx_julia + its flag against fr_render_deep_julia + its flag: the iter values that differ and the differences
    of the counts are exactly what the two restatements give on the CPU"""
    v = JB.view(name)
    it_x = _render(fr, renderer, v, W, H, extended=True)[2]
    steps_x = np.array(_steps(renderer, True), np.int64)
    it_d = _render(fr, renderer, v, W, H)[2]
    steps_d = np.array(_steps(renderer, False), np.int64)
    sx, cx, _ = JB.restated_x_bla(name)
    sd, cd, _ = JB.restated_bla(name)
    cpu = int((sx[0][0] != sd[0][0]).sum())
    gpu = int((it_x != it_d).sum())
    print(name, "iter values that differ: restatements", cpu, "GPU", gpu, "count differences", steps_x - steps_d)
    assert gpu == cpu
    assert tuple(steps_x - steps_d) == tuple(np.array(cx, np.int64) - np.array(cd, np.int64))
    assert tuple(steps_x) == tuple(cx) and steps_x[1] > 0
    assert np.array_equal(it_x, sx[0][0])


# 5. edges at 64 x 48
def _edge(fr, renderer, v, extended, w=64, h=48, aa=1):
    """flagged against the restatement (iter, nu, counts); byte-equal to the unflagged render where no BLA step is taken"""
    got = _render(fr, renderer, v, w, h, aa, True, extended)
    steps = _steps(renderer, extended)
    samples, counts = _restate(v, extended, w, h, aa)
    assert np.array_equal(got[2], samples[0][0]), int((got[2] != samples[0][0]).sum())
    assert np.abs(got[1] - J.smooth(samples[0][0], samples[0][1], v["max_iter"])).max() <= NU_TOL
    assert steps == tuple(counts), (steps, counts)
    if counts[1] == 0:
        assert _same(got, _render(fr, renderer, v, w, h, aa, True, extended, bla=False))
    return counts


@pytest.mark.parametrize("extended", [False, True], ids=["fp64", "extended"])
@pytest.mark.parametrize("c", [(0.0, 0.0), (-1.0, 0.0)], ids=["c0", "c-1"])
def test_superattracting_critical_orbits(fr, renderer, c, extended):
    """c = 0: Q is 0, 0, 0, ...; c = -1: Q is 0, -1, 0, -1, ...  Every entry of Q's table covers a zero and has r = 0: no step
    is taken on Q, whatever is taken on P.  BASILICA30's centre is alpha of c = -1; for c = 0 a centre inside the disc."""
    if c == (0.0, 0.0):
        v = dict(name="c0", c=c, cx="0.5", cy="0.25", zoom=1e-30, zoom_s="1e-30", max_iter=300, F=256)
    else:
        v = JB.view("BASILICA30")
    stats = {}
    _restate(v, extended, 64, 48, stats=stats)
    assert stats["bla_q"] == 0
    _edge(fr, renderer, v, extended, aa=2)


@pytest.mark.parametrize("extended", [False, True], ids=["fp64", "extended"])
@pytest.mark.parametrize("cx,n_p", [("2.5", 1), ("1.6", 2)])
def test_a_primary_orbit_that_escapes_at_once(fr, renderer, cx, n_p, extended):
    """N_P <= 2: no table for P, Q's is there"""
    v = dict(name="esc", c=(0.0, 1.0), cx=cx, cy="0", zoom=1e-30, zoom_s="1e-30", max_iter=200, F=256)
    P, Q = J.reference_orbits(v)
    assert len(P) - 1 == n_p and len(Q) - 1 == 200
    counts = _edge(fr, renderer, v, extended)
    assert counts[1] == 0
    L = fr.lib()
    n = (L.fr_deepx_julia_bla_table(renderer._ctx, None, None, None, 0) if extended
         else L.fr_deep_julia_bla_table(renderer._ctx, None, None, 0))
    assert n == JB.entries(200)


@pytest.mark.parametrize("extended", [False, True], ids=["fp64", "extended"])
@pytest.mark.parametrize("max_iter", [1, 2, 3, 4, 5, 6, 9, 10, 17, 18])
def test_short_orbits_and_power_of_two_lengths(fr, renderer, max_iter, extended):
    """DENDRITE30's orbits cut by max_iterations: N_P = N_Q = max_iter.  N <= 2 has no table; N - 1 a power of two has one entry
    at the top level; N - 1 one more than that leaves the last single step outside every level."""
    v = dict(JB.view("DENDRITE30"), max_iter=max_iter)
    P, Q = J.reference_orbits(v)
    assert len(P) - 1 == max_iter and len(Q) - 1 == max_iter
    counts = _edge(fr, renderer, v, extended)
    L = fr.lib()
    n = (L.fr_deepx_julia_bla_table(renderer._ctx, None, None, None, 0) if extended
         else L.fr_deep_julia_bla_table(renderer._ctx, None, None, 0))
    assert n == 2 * JB.entries(max_iter)
    if max_iter <= 2:
        assert counts[1] == 0 and n == 0
    elif max_iter >= 5:
        assert counts[1] > 0


@pytest.mark.parametrize("extended", [False, True], ids=["fp64", "extended"])
def test_the_sample_with_d0_zero(fr, renderer, extended):
    """even W and H: the centre pixel's sample has d0 = 0, its dz stays 0 on P and passes every probe with r > 0"""
    v = JB.view("DENDRITE30")
    _edge(fr, renderer, v, extended)
    d0x, d0y = S.sample_dc(64, 48, v["zoom"], 1, 0, rows=[24])
    assert d0x[0, 32] == 0.0 and d0y[0, 32] == 0.0


@pytest.mark.parametrize("extended", [False, True], ids=["fp64", "extended"])
def test_a_shallow_view(fr, renderer, extended):
    """zoom = 3: deltas of the size of the orbit, next to no probe passes"""
    _edge(fr, renderer, J.SHALLOW[0], extended, aa=2)


# 6. render paths
@pytest.mark.parametrize("extended", [False, True], ids=["fp64", "extended"])
def test_shards_layouts_memory_and_async(fr, renderer, extended):
    import torch
    v = JB.view("PRECRIT60")
    w, h = 101, 75
    ref = _render(fr, renderer, v, w, h, 2, True, extended)
    ref_steps = _steps(renderer, extended)
    assert ref_steps[1] > 0 and len(np.unique(ref[2])) > 5
    for nparts in (1, 3, 8):
        rgba = np.zeros_like(ref[0]); nu = np.zeros_like(ref[1]); it = np.full_like(ref[2], -7)
        tot = np.zeros(3, np.int64)
        for part in range(nparts):
            sh = fr.Shard(part, nparts)
            g = sh.global_rows(h)
            a, n, i = _render(fr, renderer, v, w, h, 2, True, extended, shard=sh)
            rgba[g], nu[g], it[g] = a, n, i
            if sh.rows(h):
                tot += np.array(_steps(renderer, extended))
        assert _same((rgba, nu, it), ref), nparts
        assert tuple(tot) == ref_steps, nparts                       # the counts of a call cover its own pixels
    dev = torch.device("cuda:0")
    st = _state(fr, v, 2, extended)
    view = _view(fr, v, extended)
    for sync in (True, False):
        d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
        d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
        d_it = torch.zeros((h, w), dtype=torch.int32, device=dev)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        if sync:
            renderer.render_deep_julia(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it, bla=True)
        else:
            renderer.render_deep_julia(st, w, h, view, post_chain=True, rgba=d_rgba, nu=d_nu, iter=d_it, stream=s.cuda_stream,
                                       sync=False, bla=True)
            s.synchronize()
            renderer.check()
        assert _steps(renderer, extended) == ref_steps, sync
        assert _same((d_rgba.cpu().numpy(), d_nu.cpu().numpy(), d_it.cpu().numpy()), ref), sync
    # FR_LAYOUT_FRAME: each part writes its rows in place into whole-frame device planes
    L = fr.lib()
    p = st.to_params(fr.FractalType.JuliaSet, fr.Precision.F64, True)
    p.flags |= fr.FR_FLAG_DEEPX_JULIA_BLA if extended else fr.FR_FLAG_DEEP_JULIA_BLA
    cv = view.to_cx() if extended else view.to_c()
    entry = L.fr_render_deepx_julia if extended else L.fr_render_deep_julia
    d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
    d_nu = torch.zeros((h, w), dtype=torch.float64, device=dev)
    d_it = torch.full((h, w), -7, dtype=torch.int32, device=dev)
    o = fr._capi.fr_output(d_rgba.data_ptr(), d_nu.data_ptr(), d_it.data_ptr(), fr._capi.FR_MEM_DEVICE, fr._capi.FR_LAYOUT_FRAME)
    torch.cuda.synchronize()
    for part in range(3):
        sh = fr._capi.fr_shard(part, 3, 16)
        assert entry(renderer._ctx, C.byref(p), C.byref(cv), w, h, C.byref(sh), C.byref(o)) == 0
    assert _same((d_rgba.cpu().numpy(), d_nu.cpu().numpy(), d_it.cpu().numpy()), ref)


@pytest.mark.parametrize("extended", [False, True], ids=["fp64", "extended"])
def test_a_zoom_change_reuses_the_tables_and_a_new_c_rebuilds_them(fr, extended):
    """the tables are keyed by the orbit slot alone (fr_deep_bla_builds counts the builds of a slot)"""
    L = fr.lib()
    v = dict(JB.view("DENDRITE30"), frac_bits=256)                  # F given: the automatic one follows the zoom
    assert v["F"] == 256
    w, h = 64, 48
    zooms = [("1e-30", 1e-30), ("3e-31", 3e-31), ("7e-30", 7e-30)]
    with fr.Renderer(0) as r:
        builds = lambda: L.fr_deep_bla_builds(r._ctx, int(extended), 2)
        assert builds() == 0
        _render(fr, r, v, w, h, extended=extended, bla=False)
        assert builds() == 0                                         # the unflagged path builds nothing
        frames = []
        for zs, z in zooms:                                          # one centre, one F: one build
            vz = dict(v, zoom=z, zoom_s=zs)
            frames.append(_render(fr, r, vz, w, h, extended=extended)[2])
            assert builds() == 1, zs
            assert np.array_equal(frames[-1], _restate(vz, extended, w, h, orbits=(JB.orbits_x if extended else JB.orbits)("DENDRITE30"))[0][0][0])
        assert not np.array_equal(frames[0], frames[1])
        v2 = dict(v, c=(0.0, 1.0 - 2.0 ** -30))                      # another c at the same centre strings
        it2 = _render(fr, r, v2, w, h, extended=extended)[2]
        assert builds() == 2
        assert np.array_equal(it2, _restate(v2, extended, w, h)[0][0][0])
        assert np.array_equal(_render(fr, r, v, w, h, extended=extended)[2], frames[0]) and builds() == 3


def test_neither_julia_flag_evicts_another_path(fr):
    """both Julia paths with their flags, fr_render_deep with its BLA and fr_render_deepx_ship with its BLA on one context,
    interleaved: every frame equals the same frame rendered alone, each path's counts stay its own, and no table is rebuilt"""
    import deep_ship_ref as SR
    import deepx_ship_ref as SX
    import deep_bla_ref as BR
    w, h = 64, 48
    L = fr.lib()
    sx = SX.views()["S400"]
    va = JB.view("DENDRITE30")
    vb = JB.view("DENDRITE400")

    def planes():
        return np.empty((h, w, 4), np.float32), np.empty((h, w), np.float64), np.empty((h, w), np.int32)

    def julia(r, v, extended, flag=True):
        out = _render(fr, r, v, w, h, 1, True, extended, bla=flag)
        return out + ((_steps(r, extended),) if flag else ())

    def deep_bla(r):
        out = planes()
        vc = BR.VIEW_C
        r.render_deep(fr.FractalState(zoom=vc["zoom"], max_iterations=800), w, h, fr.DeepView(vc["cx"], vc["cy"]), post_chain=True,
                      rgba=out[0], nu=out[1], iter=out[2], bla=True)
        return out + (tuple(r.last_deep_steps()),)

    def shipx_bla(r):
        out = planes()
        r.render_deepx_ship(fr.FractalState(max_iterations=sx["max_iter"]), w, h, fr.DeepView(sx["cx"], sx["cy"], zoom=sx["zoom"]),
                            post_chain=True, rgba=out[0], nu=out[1], iter=out[2], bla=True)
        return out + (tuple(r.last_deepx_ship_steps()),)

    jobs = {"Jb": lambda r: julia(r, va, False), "Jp": lambda r: julia(r, va, False, False), "Xb": lambda r: julia(r, vb, True),
            "Xp": lambda r: julia(r, vb, True, False), "Mb": deep_bla, "Sb": shipx_bla}
    alone = {}
    for key, fn in jobs.items():
        with fr.Renderer(0) as r:
            alone[key] = fn(r)
    assert alone["Jb"][3][1] > 0 and alone["Xb"][3][1] > 0
    with fr.Renderer(0) as r:
        for key in ("Jb", "Mb", "Xb", "Sb", "Jp", "Jb", "Xp", "Mb", "Xb", "Sb", "Jb"):
            got = jobs[key](r)
            for g, want in zip(got, alone[key]):
                assert np.array_equal(np.asarray(g).view(np.uint8), np.asarray(want).view(np.uint8)), key
        assert _steps(r, False) == alone["Jb"][3] and _steps(r, True) == alone["Xb"][3]
        assert tuple(r.last_deep_steps()) == alone["Mb"][3] and tuple(r.last_deepx_ship_steps()) == alone["Sb"][3]
        # one build per path: nobody's orbit or table was evicted
        assert [L.fr_deep_bla_builds(r._ctx, e, f) for e, f in ((0, 2), (1, 2), (0, 0), (1, 1))] == [1, 1, 1, 1]
