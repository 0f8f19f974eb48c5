"""The sixteen deep-view kernels over the parameters their validators accept (fr_render_deep, fr_render_deepx,
fr_render_deep_ship, fr_render_deepx_ship, fr_render_deep_julia, fr_render_deepx_julia, fr_render_deep_de, fr_render_deepx_de,
each plain and with its BLA flag), against the numpy restatements: bailout 2 .. 65536 and <= 1, reference orbits of 1, 2 and 3
updates, a critical orbit of Julia of 1 and 2, max_iterations 1, 2, 3, every palette mode, colour scale / offset, interior
style, the post chain's knobs, the distance shading, antialiasing_samples 3 and 4, and the fields of the orbit cache key.
The cases and what each of them can see are data and CPU predicates in deep_cases.py, asserted by
test_deep_cases_host.py::test_cases_can_fail; the bars are those of test_deep_gpu.py and test_deep_de_gpu.py, imported: iter
bit for bit on every pixel, nu within NU_TOL with NaN and infinities at the restatement's positions, colour within RGB_TOL on
all but _few pixels, alpha exactly 1, the step counts of the BLA paths equal, deriv bit for bit and de within DE_TOL.  Every
render goes into guard-banded planes pre-filled with a pattern no kernel produces.

316 tests: 287 cases of test_planes_match_the_restatement, then 6 + 6 + 2 + 5 + 10.
"""
import numpy as np
import pytest

import deep_cases as dc
from guarded import F64_PATTERN, GuardedPlane, GuardedPlanes
from test_deep_de_gpu import DE_TOL
from test_deep_gpu import NU_TOL, RGB_TOL, _few

pytestmark = pytest.mark.gpu

assert RGB_TOL == dc.RGB_TOL

STATE_KEYS = ("bailout", "antialiasing_samples", "palette_mode", "color_offset", "color_scale", "interior_style",
              "orbit_trap_enabled", "stripe_enabled", "color_brightness", "color_saturation", "color_contrast")
STEPS = {"deep_bla": "last_deep_steps", "de_bla": "last_deep_steps", "deepx_bla": "last_deepx_steps", "dex_bla": "last_deepx_steps",
         "ship_bla": "last_deep_ship_steps", "shipx_bla": "last_deepx_ship_steps", "julia_bla": "last_deep_julia_steps",
         "juliax_bla": "last_deepx_julia_steps"}
assert set(STEPS) == set(dc.FLAGGED)


def gpu_render(fr, r, case, frac_bits=0, c=None):
    """the case on the GPU, in guard-banded device planes: (rgba, nu, iter), then (de, deriv) on a DE path, then the step
    counts of a flagged path.  c: Julia's constant in place of the view's."""
    v = dc.view_of(case)
    q = case.params
    path = case.path
    julia = path in dc.JULIA_PATHS
    extended = path in dc.EXTENDED or path in ("juliax", "juliax_bla")
    flagged = path in dc.FLAGGED
    kw = {k: q[k] for k in STATE_KEYS if k in q}
    if not extended:
        kw["zoom"] = v["zoom"]
    if julia:
        kw["julia_c_real"], kw["julia_c_imag"] = v["c"] if c is None else c
    st = fr.FractalState(max_iterations=v["max_iter"], **kw)
    zoom_s = (v["zoom_s"] if julia else v["zoom"]) if extended else None
    view = fr.DeepView(v["cx"], v["cy"], frac_bits=frac_bits, zoom=zoom_s)
    planes = GuardedPlanes(case.H, case.W, f64=True, backend="device")
    args = (st, case.W, case.H, view)
    kwargs = dict(post_chain=bool(q.get("post", False)), **planes.kwargs())
    extra = ()
    if path in dc.DE_PATHS:
        extra = (GuardedPlane(case.H, case.W, 1, np.float64, F64_PATTERN, "device"),
                 GuardedPlane(case.H, case.W, 2, np.float64, F64_PATTERN, "device"))
        kwargs.update(de=extra[0].payload(extra[0].shape), deriv=extra[1].payload(extra[1].shape), bla=flagged)
        if "shade" in q:
            kwargs.update(shade=bool(q["shade"]), edge_px=float(q["edge_px"]))
        (r.render_deepx_de if extended else r.render_deep_de)(*args, **kwargs)
    elif path in ("ship", "ship_bla"):
        r.render_deep_ship(*args, bla=flagged, **kwargs)
    elif path in ("shipx", "shipx_bla"):
        r.render_deepx_ship(*args, bla=flagged, **kwargs)
    elif julia:
        r.render_deep_julia(*args, bla=flagged, **kwargs)
    else:
        r.render_deep(*args, bla=path == "deep_bla", xbla=path == "deepx_bla", **kwargs)
    assert planes.guards_intact(), planes.guard_hits()
    assert planes.unwritten() == 0, planes.unwritten()
    out = planes.values()
    for p in extra:
        assert p.guards_intact(), p.guard_hits()
        assert p.unwritten() == 0, p.unwritten()
        out += (p.values(p.shape),)
    if flagged:
        out += (tuple(getattr(r, STEPS[path])()),)
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
    if r.D is not None:
        de, deriv = got[3:5]
        want_deriv = dc.expected_deriv(case)
        wrong = (deriv.view(np.uint64) != want_deriv.view(np.uint64)).any(axis=2)
        assert not wrong.any(), (what, "deriv", int(wrong.sum()), "first at (y, x)", tuple(map(int, np.argwhere(wrong)[0])))
        want_de = dc.expected_de(case)
        zero = want_de == 0.0
        assert np.all(de[zero] == 0.0), (what, "de is not 0 where the restatement's is", int((de[zero] != 0.0).sum()))
        fin = ~zero & np.isfinite(want_de)
        other = ~zero & ~fin
        assert np.array_equal(de[other].view(np.uint64), want_de[other].view(np.uint64)), (what, "non-finite de")
        with np.errstate(all="ignore"):
            rel = np.abs(de[fin] - want_de[fin]) / np.abs(want_de[fin])
        worst = float(rel.max()) if fin.any() else 0.0
        print(what, "de: zeros", int(zero.sum()), "non-finite", int(other.sum()), "worst relative difference", worst, "DE_TOL", DE_TOL)
        assert not np.isnan(rel).any() and worst <= DE_TOL, (what, worst)
    if r.counts is not None:
        # every table radius and every level choice of the kernel, summed: equal, not close
        assert got[-1] == r.counts, (what, got[-1], r.counts)


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


SMALL_BLA = {"deep_bla": ("deep", "SMALL_M"), "deepx_bla": ("deepx", "SMALL_M"), "ship_bla": ("ship", "SMALL_S"),
             "shipx_bla": ("shipx", "SMALL_S"), "julia_bla": ("julia", "RABBIT30"), "juliax_bla": ("juliax", "RABBIT30")}


@pytest.mark.parametrize("path", list(SMALL_BLA))
def test_small_bailout_on_the_bla_paths(fr, renderer, oracle, path):
    """bailout 0.75 through the BLA loops: the planes of the flagged path's own restatement, and iter equal to the unflagged
    path's on every pixel (the restatements agree on 6144 of 6144, asserted first: on the Mandelbrot and ship centres no
    delta is below a table radius at this depth, the counts say so; on RABBIT30 P's table takes 24 726 steps, Q has none, and
    the skipped updates change no escape)."""
    unflagged, view = SMALL_BLA[path]
    case = dc.Case(path, view, dict(bailout=0.75), dc.W0, dc.H0)
    plain = dc.Case(unflagged, view, dict(bailout=0.75), dc.W0, dc.H0)
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


@pytest.mark.parametrize("cid", dc.GROUPS_BY_ID["julia_noop"])
def test_julia_ignores_the_styles_trap_and_stripes(fr, renderer, cid):
    """fr_deep_julia_validate accepts interior styles 1 .. 3, the orbit trap and the stripes, and nothing reads them: the planes
    are those of the defaults byte for byte"""
    on = dc.CASES[cid]
    off = dc.Case(on.path, on.view, {}, on.W, on.H)
    got, want = gpu_render(fr, renderer, on), gpu_render(fr, renderer, off)
    assert len(got) == len(want) == 3 and _same(got, want)


@pytest.mark.parametrize("path,view", [("deep", "A"), ("ship", "SHIP_A"), ("deep_bla", "A"),
                                       ("deep", "M_N3"), ("ship", "S_N3"), ("deep_bla", "M_N3"),
                                       ("julia", "RABBIT30"), ("julia_bla", "J_N3"), ("ship_bla", "S_N3"), ("shipx", dc.X_SHIP)])
def test_cache_keys(fr, path, view):
    """Every field of the orbit cache key on one context: the bailout (4, 2, 4), max_iterations (the view's, 56 fewer -- half
    of it on a view of fewer than 112 --, the view's), frac_bits (explicit and equal to the automatic value, then 64 more), and
    on Julia the bits of c (the base, c + (2^-20, 0), the base).  Each render equals the same render alone on a fresh context,
    byte for byte, the step counts of the BLA path included.  On A and SHIP_A the orbit of bailout 4 is one
    point longer than that of bailout 2 and no sample reaches the point: a key without the bailout passes there
    (test_wrong_build_5_orbit_cache_key_without_the_bailout); on the short-orbit views it rebases every surviving sample
    elsewhere."""
    v = dc.VIEWS[view]
    auto = fr.deepx_frac_bits(v["zoom"]) if path in dc.EXTENDED else fr.deep_frac_bits(v["zoom"])
    fewer = v["max_iter"] - 56 if v["max_iter"] >= 112 else v["max_iter"] // 2
    jobs = {"base": ({}, 0, None), "b2": (dict(bailout=2.0), 0, None), "mi": (dict(max_iterations=fewer), 0, None),
            "fb": ({}, auto, None), "fb64": ({}, auto + 64, None)}
    order = ("base", "b2", "base", "base", "mi", "base", "fb", "fb64", "base", "b2")
    if path in dc.JULIA_PATHS:
        jobs["c2"] = ({}, 0, (v["c"][0] + 2.0 ** -20, v["c"][1]))
        order = order[:3] + ("c2",) + order[3:]

    def run(r, key):
        params, frac_bits, c = jobs[key]
        return gpu_render(fr, r, dc.Case(path, view, params, dc.W0, dc.H0), frac_bits, c)

    alone = {}
    for key in jobs:
        with fr.Renderer(0) as r:
            alone[key] = run(r, key)
    assert _same(alone["fb"], alone["base"])
    assert not _same(alone["b2"][:3], alone["base"][:3]) and not _same(alone["mi"][:3], alone["base"][:3])
    if "c2" in jobs:
        assert not _same(alone["c2"][:3], alone["base"][:3])
    with fr.Renderer(0) as r:
        for key in order:
            got = run(r, key)
            assert _same(got, alone[key]), (path, view, key)
            assert len(got) == len(alone[key])
