"""The deep-view kernels over the parameters their validators accept (fr_render_deep, FR_FLAG_DEEP_BLA, fr_render_deepx,
FR_FLAG_DEEPX_BLA, fr_render_deep_ship), against the numpy restatements: bailout 2 .. 65536 and <= 1, reference orbits of
1, 2 and 3 updates, max_iterations 1, 2, 3, every palette mode, colour scale / offset, interior style, the post chain's
knobs, antialiasing_samples 3 and 4, and the fields of the orbit cache key.  The cases and what each of them can see are
data and CPU predicates in deep_cases.py, asserted by test_deep_cases_host.py::test_cases_can_fail; the bars are those of
test_deep_gpu.py, imported: iter bit for bit on every pixel, nu within NU_TOL with NaN and infinities at the restatement's
positions, colour within RGB_TOL on all but _few pixels, alpha exactly 1, the step counts of the BLA paths equal.  Every
render goes into guard-banded planes pre-filled with a pattern no kernel produces.

118 tests: 102 cases of test_planes_match_the_restatement, then 6 + 2 + 2 + 6.
"""
import numpy as np
import pytest

import deep_cases as dc
from guarded import GuardedPlanes
from test_deep_gpu import NU_TOL, RGB_TOL, _few

pytestmark = pytest.mark.gpu

assert RGB_TOL == dc.RGB_TOL

STATE_KEYS = ("bailout", "antialiasing_samples", "palette_mode", "color_offset", "color_scale", "interior_style",
              "stripe_enabled", "color_brightness", "color_saturation", "color_contrast")


def gpu_render(fr, r, case, frac_bits=0):
    """the case on the GPU, in guard-banded device planes; (rgba, nu, iter[, step counts of a BLA path])"""
    v = dc.view_of(case)
    q = case.params
    extended = case.path in ("deepx", "deepx_bla")
    kw = {k: q[k] for k in STATE_KEYS if k in q}
    if not extended:
        kw["zoom"] = v["zoom"]
    st = fr.FractalState(max_iterations=v["max_iter"], **kw)
    view = fr.DeepView(v["cx"], v["cy"], frac_bits=frac_bits, zoom=v["zoom"] if extended else None)
    planes = GuardedPlanes(case.H, case.W, f64=True, backend="device")
    post = bool(q.get("post", False))
    if case.path == "ship":
        r.render_deep_ship(st, case.W, case.H, view, post_chain=post, **planes.kwargs())
    else:
        r.render_deep(st, case.W, case.H, view, post_chain=post, bla=case.path == "deep_bla",
                      xbla=case.path == "deepx_bla", **planes.kwargs())
    assert planes.guards_intact(), planes.guard_hits()
    assert planes.unwritten() == 0, planes.unwritten()
    out = planes.values()
    if case.path == "deep_bla":
        out += (tuple(r.last_deep_steps()),)
    elif case.path == "deepx_bla":
        out += (tuple(r.last_deepx_steps()),)
    return out


def nu_mismatches(nu, want):
    """pixels whose nu is neither the restatement's value (an infinity included), nor NaN where it is NaN, nor within NU_TOL"""
    with np.errstate(invalid="ignore"):
        ok = (nu == want) | (np.isnan(nu) & np.isnan(want)) | (np.abs(nu - want) <= NU_TOL)
    return ~ok


def rgb_mismatches(rgb, want):
    with np.errstate(invalid="ignore"):
        ok = (np.abs(rgb - want) <= RGB_TOL) | (np.isnan(rgb) & np.isnan(want))
    return ~ok.all(axis=2)


def check(oracle, case, got, what):
    rgba, nu, it = got[:3]
    r = dc.restated(case)
    r_it = r.samples[0][0]                                          # iter and nu are those of sample 0
    wrong = it != r_it
    assert not wrong.any(), (what, int(wrong.sum()), "first at (y, x)", tuple(map(int, np.argwhere(wrong)[0])),
                             "gpu", int(it[wrong][0]), "restated", int(r_it[wrong][0]))
    want_nu = dc.expected_nu(case)
    bad_nu = nu_mismatches(nu, want_nu)
    with np.errstate(invalid="ignore"):
        print(what, "nu: NaN", int(np.isnan(want_nu).sum()), "inf", int(np.isinf(want_nu).sum()), "largest finite difference",
              float(np.nanmax(np.where(np.isfinite(nu - want_nu), np.abs(nu - want_nu), 0.0))))
    assert not bad_nu.any(), (what, int(bad_nu.sum()), "first", float(nu[bad_nu][0]), float(want_nu[bad_nu][0]))
    assert np.all(rgba[..., 3] == 1.0), what
    bad = rgb_mismatches(rgba[..., :3], dc.expected_rgb(oracle, case))
    print(what, "rgb outside tolerance", int(bad.sum()), "of", bad.size)
    assert _few(bad, bad.size), (what, int(bad.sum()))
    if r.counts is not None:
        # every table radius and every level choice of the kernel, summed: equal, not close
        assert got[3] == r.counts, (what, got[3], r.counts)


@pytest.mark.parametrize("cid", list(dc.CASES))
def test_planes_match_the_restatement(fr, renderer, oracle, cid):
    case = dc.CASES[cid]
    check(oracle, case, gpu_render(fr, renderer, case), cid)


# fr_render in fp64 at the same (exactly representable) centre computes the same orbits by other roundings.  The bar is the
# agreement of the RESTATEMENT with oracle.render on the CPU less 0.01: measured 1.0 (6144 of 6144) on M_N1, M_N2, M_N3,
# S_N1 and S_N2, 0.99495 (31 pixels differ) on S_N3, so 0.99 and 0.98495 -- within the 0.98 .. 0.99 of the shallow-view
# tests of test_deep_gpu.py and test_deep_ship_gpu.py.
FR_RENDER_BAR = {"M_N1": 0.99, "M_N2": 0.99, "M_N3": 0.99, "S_N1": 0.99, "S_N2": 0.99, "S_N3": 0.98495}


@pytest.mark.parametrize("cid", ["short/deep-M_N1", "short/deep-M_N2", "short/deep-M_N3",
                                 "short/ship-S_N1", "short/ship-S_N2", "short/ship-S_N3"])
def test_short_orbits_agree_with_fr_render(fr, renderer, cid):
    case = dc.CASES[cid]
    v = dc.view_of(case)
    it = gpu_render(fr, renderer, case)[2]
    st = fr.FractalState(center_x=float(v["cx"]), center_y=float(v["cy"]), zoom=v["zoom"], max_iterations=v["max_iter"])
    planes = GuardedPlanes(case.H, case.W, f64=True, backend="device", planes=("iter",))
    renderer.render(st, case.W, case.H, precision=fr.Precision.F64, **planes.kwargs(),
                    fractal_type=fr.FractalType.BurningShip if case.path == "ship" else fr.FractalType.Mandelbrot)
    assert planes.guards_intact() and planes.unwritten() == 0
    it64 = planes.values()[2]
    agreement = float((it == it64).mean())
    print(cid, "agreement with fr_render", agreement, "bar", FR_RENDER_BAR[case.view])
    assert agreement >= FR_RENDER_BAR[case.view]


@pytest.mark.parametrize("path", ["deep_bla", "deepx_bla"])
def test_small_bailout_on_the_bla_paths(fr, renderer, oracle, path):
    """bailout 0.75 on the Mandelbrot centre through both BLA loops: the planes of the flagged path's own restatement, and
    iter equal to the unflagged path's on every pixel (the restatements agree on 6144 of 6144: at this depth no delta is
    below a table radius, the counts say so)."""
    case = dc.Case(path, "SMALL_M", dict(bailout=0.75), dc.W0, dc.H0)
    plain = dc.Case("deep" if path == "deep_bla" else "deepx", "SMALL_M", dict(bailout=0.75), dc.W0, dc.H0)
    assert np.array_equal(dc.restated(case).samples[0][0], dc.restated(plain).samples[0][0])
    got = gpu_render(fr, renderer, case)
    check(oracle, case, got, path)
    assert np.array_equal(got[2], gpu_render(fr, renderer, plain)[2])


def _same(got, want):
    return all(np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)) for g, w in zip(got, want))


@pytest.mark.parametrize("style", [0, 1])
def test_ship_stripes_without_style_2_change_nothing(fr, renderer, style):
    on = dc.CASES[f"ship_noop/ship-stripes-interior{style}"]
    off = dc.Case(on.path, on.view, dict(on.params, stripe_enabled=False), on.W, on.H)
    assert _same(gpu_render(fr, renderer, on), gpu_render(fr, renderer, off))


@pytest.mark.parametrize("path,view", [("deep", "A"), ("ship", "SHIP_A"), ("deep_bla", "A"),
                                       ("deep", "M_N3"), ("ship", "S_N3"), ("deep_bla", "M_N3")])
def test_cache_keys(fr, path, view):
    """Every field of the orbit cache key on one context: the bailout (4, 2, 4), max_iterations (the view's, 56 fewer, the
    view's), frac_bits (explicit and equal to the automatic value, then 64 more).  Each render equals the same render alone on
    a fresh context, byte for byte, the step counts of the BLA path included.  On A and SHIP_A the orbit of bailout 4 is one
    point longer than that of bailout 2 and no sample reaches the point: a key without the bailout passes there
    (test_wrong_build_5_orbit_cache_key_without_the_bailout); on the short-orbit views it rebases every surviving sample
    elsewhere."""
    v = dc.VIEWS[view]
    auto = fr.deep_frac_bits(v["zoom"])
    jobs = {"base": ({}, 0), "b2": (dict(bailout=2.0), 0), "mi": (dict(max_iterations=v["max_iter"] - 56), 0),
            "fb": ({}, auto), "fb64": ({}, auto + 64)}

    def run(r, key):
        params, frac_bits = jobs[key]
        return gpu_render(fr, r, dc.Case(path, view, params, dc.W0, dc.H0), frac_bits)

    alone = {}
    for key in jobs:
        with fr.Renderer(0) as r:
            alone[key] = run(r, key)
    assert _same(alone["fb"], alone["base"])
    assert not _same(alone["b2"][:3], alone["base"][:3]) and not _same(alone["mi"][:3], alone["base"][:3])
    with fr.Renderer(0) as r:
        for key in ("base", "b2", "base", "base", "mi", "base", "fb", "fb64", "base", "b2"):
            got = run(r, key)
            assert _same(got, alone[key]), (path, view, key)
            assert len(got) == len(alone[key])
