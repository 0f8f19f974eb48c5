"""The deep parameter cases (tests/deep_cases.py) on the CPU: what each case can see, the restatements against the exact
integer iteration across the bailout range, and eight deliberately wrong builds of the argument blocks / the orbit cache,
emulated in numpy with the restatement in place of the kernel -- each must fail at least one case of the table, the last
three cases that the table of the first five paths did not have.  No GPU, no product library: numpy, Python integers and
the CPU oracle's colour stage."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import deep_cases as dc
import deep_julia_bla_ref as JB
import deep_julia_ref as J
import deep_ref as R
import deep_ship_ref as S
import deepx_ref as X

NU_TOL = 1e-9                         # test_deep_gpu.NU_TOL (asserted equal in test_deep_cases_gpu.py)
RGB_TOL = dc.RGB_TOL


def _few(bad, n):
    """test_deep_gpu._few"""
    return int(bad.sum()) <= max(2, int(0.001 * n))


def _default_of(case, *drop):
    """the same case with the named parameters at their defaults"""
    return dc.Case(case.path, case.view, {k: v for k, v in case.params.items() if k not in drop}, case.W, case.H)


# ---- 1. every case can fail ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(dc.CASES))
def test_cases_can_fail(oracle, cid):
    case, group = dc.CASES[cid], dc.GROUP_OF[cid]
    v = dc.view_of(case)
    r = dc.restated(case)
    it = r.samples[0][0]
    n = it.size
    max_iter = v["max_iter"]
    escaped = float((it < max_iter).mean())
    classes, sizes = np.unique(it, return_counts=True)
    print(cid, "N", r.N, "classes", len(classes), "largest", sizes.max() / n, "escaped", escaped, "counts", r.counts)
    assert it.shape == (case.H, case.W)
    if group == "bailout":
        # as the probe of test_restatement_agrees_with_exact_iteration_across_bailout, on this frame; and the bailout is
        # visible: most samples that escape under both escape at another update than under the default
        assert 0.20 <= escaped <= 0.95
        it4 = dc.restated(_default_of(case, "bailout")).samples[0][0]
        both = (it < max_iter) & (it4 < max_iter)
        assert (it[both] != it4[both]).mean() >= 0.25
    elif group == "small":
        assert sizes.max() / n <= 0.70 and len(classes) >= 2 and r.N >= 6          # (Julia: N is N_P)
        assert not (np.float32(dc.bailout_of(case)) > np.float32(1.0))             # the lib_log branch
        assert len(classes[classes < max_iter]) >= 2                               # escapes at two different updates
        want_nq = dc.SMALL_NQ.get((case.view, dc.bailout_of(case)))
        if want_nq is not None:
            assert case.path in dc.JULIA_PATHS and r.NQ == want_nq and r.NQ <= 2
            if case.path == "julia":                                               # samples walk the short Q, or none leaves P
                walked = r.stats["moved"][0] > 0.0
                print("share of the samples that leave P for Q", r.stats["moved"][0])
                assert walked == ((case.view, dc.bailout_of(case)) != ("DENDRITE30", 0.75))
        if case.path in ("julia_bla", "juliax_bla") and case.view == "RABBIT30" and dc.bailout_of(case) == 0.75:
            assert r.stats["bla_q"] == 0 and r.stats["bla_p"] > 0                  # Q has no table, P's alone takes steps
    elif group == "short":
        assert r.N == dc.SHORT_N[case.view]
        assert 0.05 <= 1.0 - escaped <= 0.95
        surviving = int((it == max_iter).sum())
        rb = dc.rebases_of(case)
        print("rebases", rb, "bar", surviving * max_iter / r.N * 0.9)
        assert rb >= surviving * max_iter / r.N * 0.9
        if case.path in ("julia_bla", "juliax_bla"):
            print("BLA steps on P", r.stats["bla_p"], "on Q", r.stats["bla_q"])
            if r.N <= 2:
                assert r.stats["bla_p"] == 0                                       # an orbit of one or two updates has no table
    elif group == "max_iter" and case.path in dc.JULIA_PATHS:
        # a shallow frame whose centre lies near the escape radius: samples escape at update 0, 1, .. and survive, all in one
        # frame, so a loop that runs once too often or once too few moves a whole class of iter
        assert max_iter in (1, 2, 3) and len(classes) >= max_iter + 1
        assert sizes.min() / n >= 0.05
        assert list(classes) == list(range(max_iter + 1))                          # updates 0 .. max_iter - 1, and the survivors
        if r.counts is not None:
            assert r.counts[0] + r.counts[2] == J.lane_updates(it, max_iter)
    elif group == "max_iter":
        # nothing escapes in three updates of these views: the planes are constant, and what a loop that runs once too
        # often or not at all changes is the step counts of the BLA paths (every sample: max_iter updates, no more)
        assert r.N == max_iter and escaped == 0.0
        if r.counts is not None:
            assert r.counts[0] + r.counts[2] == n * max_iter
    elif group == "colour":
        assert 1.0 - escaped >= 0.10 and escaped >= 0.50
        want = dc.expected_rgb(oracle, case)
        base = dc.expected_rgb(oracle, case, dc.default_params(case))
        diff = dc.differing(want, base)
        kind = dc.colour_expectation(case)
        print(kind, "pixels that differ from the default plane", float(diff.mean()))
        if kind == "differs":
            assert diff.mean() >= 0.25
        elif kind == "interior":
            assert np.array_equal(diff, it == max_iter)                            # every interior pixel, no other
        else:
            assert np.array_equal(want.view(np.uint32), base.view(np.uint32))
    elif group == "aa":
        assert case.W % 8 and case.H % 8                                           # ragged: lanes without a pixel
        want = dc.expected_rgb(oracle, case)
        one = dc.expected_rgb(oracle, dc.Case(case.path, case.view, dict(case.params, antialiasing_samples=1), case.W, case.H))
        # the average is not sample 0's colour: a kernel that shaded sample 0 alone would miss RGB_TOL on twenty times the
        # pixels _few lets pass
        assert int(dc.differing(want, one, RGB_TOL).sum()) >= 20 * max(2, int(0.001 * n))
        its = np.stack([s[0] for s in r.samples])
        assert (its != its[0]).any(axis=0).mean() >= 0.10                          # the samples of a pixel differ in iter
    elif group == "ship_noop":
        assert case.params["stripe_enabled"] and case.params["interior_style"] != 2
        assert 1.0 - escaped >= 0.10 and escaped >= 0.50
    elif group == "julia_noop":
        assert case.path == "julia" and any(case.params.get(k) for k in ("interior_style", "orbit_trap_enabled", "stripe_enabled"))
        assert 1.0 - escaped >= 0.10 and escaped >= 0.50
        # Julia's shader has no styles: the expected colours are those of the defaults, bit for bit
        assert np.array_equal(dc.expected_rgb(oracle, case).view(np.uint32), dc.expected_rgb(oracle, case, {}).view(np.uint32))
    else:
        raise AssertionError(group)


def test_the_table_holds_what_the_groups_promise():
    assert len(dc.CASES) == sum(len(g) for g in dc.GROUPS.values())
    paths = {g: {c.path for c in cases.values()} for g, cases in dc.GROUPS.items()}
    julia = set(dc.JULIA_PATHS)
    assert paths["bailout"] == set(dc.PATHS)
    assert paths["small"] == {"deep", "ship", "ship_bla", "shipx", "shipx_bla", "dex"} | julia
    assert paths["short"] == {"deep", "deep_bla", "deepx", "deepx_bla", "ship", "ship_bla", "shipx"} | julia
    assert paths["max_iter"] == {"deep", "deep_bla", "ship", "deepx_bla", "ship_bla", "shipx_bla", "dex_bla", "de"} | julia
    assert paths["colour"] == {"deep", "deepx", "ship", "julia", "dex_bla", "de"}
    assert paths["aa"] == {"deep", "ship", "julia", "juliax_bla", "shipx", "dex"}
    for path in ("deep", "deepx", "ship", "julia", "dex_bla", "de"):
        for shaded in (False, True):
            kinds = [dc.colour_expectation(c) for c in dc.GROUPS["colour"].values()
                     if c.path == path and "palette_mode" in c.params and bool(c.params.get("shade")) == shaded]
            if kinds:
                assert kinds.count("differs") >= 5                                  # every defined palette beside mode 0
    shaded = [c for c in dc.GROUPS["colour"].values() if c.params.get("shade")]
    assert {c.path for c in shaded} == {"dex_bla", "de"} and all(c.params["edge_px"] == 1.8 for c in shaded)
    assert all(c.params.get("shade") for c in dc.GROUPS["aa"].values() if c.path == "dex")
    # the Julia edges, each a case: N_Q of 1 and of 2, N_P of 1, 2 and 3, max_iterations 1 to 3 on all four kernels
    for path in julia:
        assert {dc.SMALL_NQ.get((c.view, dc.bailout_of(c))) for c in dc.GROUPS["small"].values() if c.path == path} == {1, 2, None}
    for path in julia:
        assert {dc.SHORT_N[c.view] for c in dc.GROUPS["short"].values() if c.path == path} == {1, 2, 3}
        assert {c.params["max_iterations"] for c in dc.GROUPS["max_iter"].values() if c.path == path} == {1, 2, 3}
    for c in dc.CASES.values():
        assert c.view not in ("E", "DENDRITE1000", "TIP1000")


def test_every_kernel_of_the_family_runs_in_some_case():
    """The table's paths are sixteen distinct deep_kernel instantiations, one per path (dc.KERNELS: deep_kernel_name of
    fr_device.hip), and every path has cases: every block fr_device.hip's entry points name (an alias of DeepBlock<F, X, DE>),
    without and with its table, but the four of Julia's distance estimate"""
    assert len(dc.PATHS) == 16 and len(set(dc.KERNELS.values())) == 16
    kernels = {dc.KERNELS[c.path] for c in dc.CASES.values()}
    assert kernels == set(dc.KERNELS.values())
    assert sum(k.startswith("deep_kernel<") for k in kernels) == 16
    import os, re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fractalrenderer_amd", "csrc",
                            "fr_device.hip")).read()
    alias = {a: (f, x == "true", de == "true")
             for a, f, x, de in re.findall(r"using (\w+) = DeepBlock<(\w+)Formula, (true|false), (true|false)>;", src)}
    assert set(re.findall(r"deep_entry<(\w+)>\(", src)) == set(alias) and len(alias) == 10
    assert '"deep_kernel<"' in src and '", X"' in src and '", DE"' in src and '", BLA"' in src
    named = {"deep_kernel<%s%s%s%s>" % (f, ", X" if x else "", ", DE" if de else "", ", BLA" if bla else "")
             for f, x, de in alias.values() for bla in (False, True)}
    assert len(named) == 20 and named - {k for k in named if k.startswith("deep_kernel<Julia") and ", DE" in k} == set(dc.KERNELS.values())


# ---- 2. the restatements are ground truth across the bailout range ---------------------------------------------------------
PW, PH = 64, 48


@functools.lru_cache(maxsize=None)
def _pixels():
    rng = np.random.default_rng(20240607)
    return rng.integers(0, PH, 48), rng.integers(0, PW, 48)


def _probe(path, view, bailout):
    """(iter plane, rebases, exact iter of the 48 pixels) of a 64 x 48 frame"""
    case = dc.Case(path, view, dict(bailout=bailout), PW, PH)
    v = dc.view_of(case)
    ys, xs = _pixels()
    if path == "deepx":
        stats = {}
        it = X.restate_x(v, PW, PH, 1, bailout, stats=stats)[0][0]
        rb = stats["rebases"]
        ex = [X.exact_iter_x(v, int(x), int(y), PW, PH, bailout=bailout) for x, y in zip(xs, ys)]
    else:
        mod = S if path == "ship" else R
        out = mod.restate(v, PW, PH, 1, bailout)
        it, rb = out[0][0][0], out[1]
        ex = [mod.exact_iter(v["cx"], v["cy"], int(x), int(y), PW, PH, v["zoom"], v["max_iter"], bailout) for x, y in zip(xs, ys)]
    return it, rb, np.array(ex)


# 128 for the probe's 100: exact as a float.  Every view passes every predicate at 2, 128 and 65536 (no bailout replaced).
@pytest.mark.parametrize("bailout", dc.BAILOUTS)
@pytest.mark.parametrize("path,view", [("deep", "A"), ("ship", "SHIP_A"), ("deepx", "D")])
def test_restatement_agrees_with_exact_iteration_across_bailout(path, view, bailout):
    it, rb, ex = _probe(path, view, bailout)
    ys, xs = _pixels()
    agreement = float((it[ys, xs] == ex).mean())
    escaped = float((it < dc.VIEWS[view]["max_iter"]).mean())
    print(path, view, bailout, "agreement", agreement, "escaped", escaped, "rebases", rb)
    assert agreement >= 0.99
    assert 0.20 <= escaped <= 0.95
    assert rb >= 4096


@pytest.mark.parametrize("path,view,bailout", [("deep", "SMALL_M", 0.75), ("ship", "SMALL_S", 0.75), ("deep", "UNIT_M", 0.75),
                                               ("ship", "UNIT_S", 0.75), ("deep", "UNIT_M", 1.0), ("ship", "UNIT_S", 1.0)])
def test_small_bailout_centres_agree_with_exact_iteration(path, view, bailout):
    it, _, ex = _probe(path, view, bailout)
    ys, xs = _pixels()
    agreement = float((it[ys, xs] == ex).mean())
    print(path, view, bailout, "agreement", agreement, "classes of the 48 pixels", np.unique(ex))
    assert agreement >= 0.99
    assert len(np.unique(ex)) >= 2


@pytest.mark.parametrize("view,bailout", [("RABBIT30", 0.75), ("DENDRITE30", 0.75), ("DUST30", 0.75), ("RABBIT30", 1.0),
                                          ("DENDRITE30", 1.0), ("J_N1", 4.0), ("J_N2", 4.0), ("J_N3", 4.0)])
def test_julia_views_agree_with_exact_iteration(view, bailout):
    """the Julia views of the small and short cases, fp64 and extended restatement, against the direct iteration in integers
    on the 48 pixels of a 64 x 48 frame; the bar of the two tests above"""
    v = dict(dc.VIEWS[view])
    ys, xs = _pixels()
    ex = np.array([J.exact_iter(v, int(x), int(y), PW, PH, bailout) for x, y in zip(xs, ys)])
    it = J.restate(v, PW, PH, 1, bailout)[0][0]
    itx = J.restate_x(v, PW, PH, 1, bailout)[0][0]
    agreement = float((it[ys, xs] == ex).mean())
    print(view, bailout, "agreement", agreement, "classes of the 48 pixels", np.unique(ex))
    assert agreement >= 0.99 and float((itx[ys, xs] == ex).mean()) >= 0.99
    assert len(np.unique(ex)) >= 2


def test_the_level_curves_are_not_resolved_at_zoom_1e_30():
    """why SMALL_ZOOM is 1e-12: at 1e-30 dz is absorbed by Z_m in the escape test, the restatement gives the whole frame
    one class and the exact iteration another for about half of it"""
    v = dict(dc._offset(dc._SMALL_M0, 1e-30), zoom=1e-30, max_iter=64)
    it = R.restate(v, PW, PH, 1, 0.75)[0][0][0]
    ys, xs = _pixels()
    ex = np.array([R.exact_iter(v["cx"], v["cy"], int(x), int(y), PW, PH, 1e-30, 64, 0.75) for x, y in zip(xs, ys)])
    assert len(np.unique(it)) == 1 and len(np.unique(ex)) >= 2
    assert (it[ys, xs] == ex).mean() <= 0.75


# ---- 3. five wrong builds, the restatement in place of the kernel ------------------------------------------------------------
def _nu_fails(got, want):
    """the nu assertion of test_deep_cases_gpu.py"""
    with np.errstate(invalid="ignore"):
        ok = (got == want) | (np.isnan(got) & np.isnan(want)) | (np.abs(got - want) <= NU_TOL)
    return not ok.all()


def _rgb_fails(got, want):
    """the rgb assertion of test_deep_cases_gpu.py"""
    with np.errstate(invalid="ignore"):
        ok = (np.abs(got - want) <= RGB_TOL) | (np.isnan(got) & np.isnan(want))
    return not _few(~ok.all(axis=2), ok.shape[0] * ok.shape[1])


def _rgb_of_nu(oracle, case, nus, shader=None):
    """dc.expected_rgb on given nu planes (one per sample); shader: the palette table of another shader (0: Mandelbrot's)"""
    v = dc.view_of(case)
    q = case.params
    ship = case.path == "ship"
    aa = dc.aa_of(case)
    p = oracle.OracleParams(fractal=2 if ship else 0, max_iterations=v["max_iter"], zoom=1.0, aa=aa, post_chain=0,
                            palette_mode=int(q.get("palette_mode", 0)), color_scale=float(q.get("color_scale", 1.0)),
                            color_offset=float(q.get("color_offset", 0.0)), interior_style=int(q.get("interior_style", 0)))
    acc = np.zeros((case.H, case.W, 3), np.float32)
    for nu in nus:
        if shader is None:
            acc = acc + oracle.colorize(p, nu)[..., :3]
        else:                               # the ship's t = offset + nu / max_iter * scale, fract in double, the other table
            t = np.float64(np.float32(p.color_offset)) + (nu / np.float64(v["max_iter"])) * np.float64(np.float32(p.color_scale))
            t = (t - np.floor(t)).astype(np.float32)
            rgb = np.array([oracle.palette(shader, p.palette_mode, float(x)) for x in t.ravel()], np.float32)
            rgb[(nu == v["max_iter"]).ravel()] = 0.0
            acc = acc + rgb.reshape(case.H, case.W, 3)
    if aa > 1:
        acc = acc / np.float32(aa * aa)
    if q.get("post", False):
        b, s, c = (float(q.get(k, 1.0)) for k in ("color_brightness", "color_saturation", "color_contrast"))
        acc = np.array([oracle.post_chain(px, b, s, c, julia_floors=int(ship)) for px in acc.reshape(-1, 3)],
                       np.float32).reshape(case.H, case.W, 3)
    return acc


@functools.lru_cache(maxsize=None)
def _log2_table():
    """the table of log2_tab (fr_ctx_create): bin i of [0.5, 1) -> (RN(1 / m_i), -log2 of that in long double, rounded)"""
    m = 0.5 + (np.arange(128, dtype=np.float64) + 0.5) / 256.0
    y = 1.0 / m
    return y, (-np.log2(y.astype(np.longdouble))).astype(np.float64)


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))           # exact, then one rounding


def _log2_tab(x):
    """log2_tab (fr_kernels.hip.h) of one positive finite double, operation for operation"""
    y, L = _log2_table()
    m, e = math.frexp(x)
    i = (int(np.float64(m).view(np.uint64)) >> 45) & 127
    r = _fma(m, y[i], -1.0)
    p = 0.28853900817779268
    for c in (-0.36067376022224085, 0.48089834696298783, -0.72134752044448170, 1.4426950408889634):
        p = _fma(p, r, c)
    return _fma(p, r, float(e) + L[i])


def test_log2_tab_emulation_is_a_log2():
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.uniform(1.0, 70000.0, 200), 1.0 + rng.uniform(0, 1e-9, 50), [1.0, 2.0, 4.0, 0.5, 3.0e-5]])
    assert max(abs(_log2_tab(float(x)) - math.log2(float(x))) for x in xs) < 4e-15


def _failing(cases, fails):
    bad = [cid for cid in cases if fails(cid, dc.CASES[cid])]
    print(len(bad), "of", len(cases), "cases fail:", bad[:8], "..." if len(bad) > 8 else "")
    return bad


def test_wrong_build_1_inv_log2_bailout_fixed_at_bailout_4(oracle):
    """a.inv_log2_bailout = 1 / log2(4): read by shade<double, 2> alone, so the ship's cases at another bailout > 1 see it"""
    def fails(cid, case):
        if case.path != "ship" or not (np.float32(dc.bailout_of(case)) > np.float32(1.0)):
            return False                                              # the field is not read
        it, r2 = dc.restated(case).samples[0]
        return _nu_fails(S.smooth(it, r2, dc.view_of(case)["max_iter"], 4.0), dc.expected_nu(case))
    bad = _failing(list(dc.CASES), fails)
    assert sorted(bad) == sorted("bailout/" + c for c in dc.GROUPS["bailout"] if c.startswith("ship-"))
    assert len(bad) == 3


def test_wrong_build_2_colour_scale_and_offset_swapped(oracle):
    """a.color_scale_d = offset, a.color_offset_d = scale: the defaults (1, 0) are not symmetric either, so every case
    with escaped samples sees it"""
    def fails(cid, case):
        q = dict(case.params, color_scale=case.params.get("color_offset", 0.0), color_offset=case.params.get("color_scale", 1.0))
        return _rgb_fails(dc.expected_rgb(oracle, case, q), dc.expected_rgb(oracle, case))
    bad = _failing(list(dc.GROUPS_BY_ID["colour"]) + list(dc.GROUPS_BY_ID["ship_noop"]) + list(dc.GROUPS_BY_ID["aa"]), fails)
    assert len(bad) >= len(dc.GROUPS["colour"]) - 3                   # all but at most the interior-only differences
    assert all(("colour/%s-scale%g-offset%g" % (path, sc, off)) in bad for path in ("deep", "deepx", "ship")
               for sc, off in (dc.SCALE_OFFSET_SHIP if path == "ship" else dc.SCALE_OFFSET))


def test_wrong_build_3_mandelbrot_palette_table_for_the_ship(oracle):
    """fr_palette_table_build(0, ..) for FR_FRACTAL_BURNING_SHIP"""
    def fails(cid, case):
        nus = [dc.smooth(case, it, r2) for it, r2 in dc.restated(case).samples]
        return _rgb_fails(_rgb_of_nu(oracle, case, nus, shader=0), dc.expected_rgb(oracle, case))
    ship = [cid for cid in dc.GROUPS_BY_ID["colour"] if dc.CASES[cid].path == "ship"]
    # the emulation of the right build is the oracle's colour stage: first that _rgb_of_nu with the ship's own table is it
    for cid in ship[:3]:
        case = dc.CASES[cid]
        nus = [dc.smooth(case, it, r2) for it, r2 in dc.restated(case).samples]
        assert not _rgb_fails(_rgb_of_nu(oracle, case, nus, shader=1), dc.expected_rgb(oracle, case)), cid
    bad = _failing(ship, fails)
    assert len(bad) >= 1
    print("ship colour cases a Mandelbrot table passes:", sorted(set(ship) - set(bad)))


def test_wrong_build_4_lib_log_taken_as_bailout_below_1(oracle):
    """a.lib_log = bailout < 1: at bailout 1 exactly the table log2 runs in place of the library log.  Both compute the same
    function; the table's error is absolute (1e-16), and log2(r2) of the samples that escape on the level curve |z_k| = 1 is
    1e-10: nu is wrong from the sixth digit.  For the ship and Julia both branches give -inf at bailout 1 (log 1 = 0 divides)."""
    def fails(cid, case):
        if dc.bailout_of(case) != 1.0:
            return False                                              # the branch taken is the same
        it, r2 = dc.restated(case).samples[0]
        want = dc.expected_nu(case)
        got = want.copy()
        e = it < dc.view_of(case)["max_iter"]
        if dc.formula(case.path) != 0:                                # lg.log2(lg.log2(r2) * (1 / log2(1)))
            got[e] = [(i + 1.0) - math.log2(_log2_tab(float(x)) * math.inf) for i, x in zip(it[e], r2[e])]
        else:
            got[e] = [(i + 1.0) - _log2_tab(0.5 * _log2_tab(float(x))) for i, x in zip(it[e], r2[e])]
        return _nu_fails(got, want)
    bad = _failing(list(dc.CASES), fails)
    assert bad == ["small/deep-UNIT_M-b1", "small/dex-UNIT_M-b1"]


def test_wrong_build_5_orbit_cache_key_without_the_bailout():
    """The second render of test_cache_keys' sequence (bailout 4, then 2) reuses the orbit of bailout 4.  On view A and on
    SHIP_A that orbit is one point longer and no sample reaches the point: the planes are the right ones, bit for bit, and
    the sequence of the issue alone would pass.  On the short-orbit views N is 3 for 2: every surviving sample rebases
    elsewhere, and r2 -- so nu -- differs in its last bits."""
    def stale_differs(mod, v):
        old = mod.reference_orbit(v["cx"], v["cy"], v["zoom"], v["max_iter"], 4.0)
        new = mod.reference_orbit(v["cx"], v["cy"], v["zoom"], v["max_iter"], 2.0)
        a = mod.restate(v, dc.W0, dc.H0, 1, 2.0, orbit=old)[0][0]
        b = mod.restate(v, dc.W0, dc.H0, 1, 2.0, orbit=new)[0][0]
        return int((a[0] != b[0]).sum()) + int((a[1].view(np.uint64) != b[1].view(np.uint64)).sum())
    got = {name: stale_differs(mod, dc.VIEWS[name]) for mod, name in ((R, "A"), (S, "SHIP_A"), (R, "M_N3"), (S, "S_N3"))}
    print(got)
    assert got["A"] == 0 and got["SHIP_A"] == 0
    assert got["M_N3"] >= 10 and got["S_N3"] >= 10


# ---- 4. three wrong builds that the table of the first five paths could not see -----------------------------------------------
def test_wrong_build_6_log_bailout_left_zero_in_a_non_mandelbrot_block(oracle):
    """log(bailout) reaches the eight ship and Julia kernels through eight ship_log_bailout overloads, a flagged kernel's from
    the base block copied into {base block, table} (launch_deep).  A block whose field stays 0: shade<double, 1> and
    shade<double, 2> read it in the lib_log branch alone, nu = (it + 1) - log(log(r2) / 0) / ln 2 -- NaN for r2 < 1, -inf for
    r2 > 1, where the right build divides by log(0.75) < 0 and is finite for r2 < 1.  At bailout 1 exactly log(bailout) IS 0:
    the builds coincide, so the cases that fail are the ship-family and Julia small cases below 1, and no other.  Of the
    eight paths the old table ran one."""
    ln2 = np.log(np.float64(2.0))

    def fails(cid, case):
        if dc.formula(case.path) == 0 or np.float32(dc.bailout_of(case)) > np.float32(1.0):
            return False                                              # Mandelbrot's shade<double, 0> has no such field; not lib_log
        it, r2 = dc.restated(case).samples[0]
        got = dc.expected_nu(case).copy()
        e = it < dc.view_of(case)["max_iter"]
        with np.errstate(all="ignore"):
            got[e] = (it[e].astype(np.float64) + 1.0) - np.log(np.log(r2[e]) / np.float64(0.0)) / ln2
        return _nu_fails(got, dc.expected_nu(case))
    bad = _failing(list(dc.CASES), fails)
    want = [cid for cid in dc.GROUPS_BY_ID["small"] if dc.formula(dc.CASES[cid].path) != 0 and dc.bailout_of(dc.CASES[cid]) < 1.0]
    assert sorted(bad) == sorted(want)
    assert {dc.CASES[cid].path for cid in bad} == set(dc.SHIP_PATHS) | set(dc.JULIA_PATHS)
    assert {dc.CASES[cid].path for cid in bad} & set(dc.OLD_PATHS) == {"ship"}


def test_wrong_build_7_julia_tables_swapped():
    """P's lanes given Q's table (its n1 / K and entries) and Q's lanes P's, on the two flagged Julia kernels: the stepping of
    deep_julia_bla_ref with the pair of tables swapped.  On RABBIT30 at bailout 0.75 Q has no table, so P's lanes take none of
    their 24 726 steps: the counts differ.  The old table had no Julia case."""
    def fails(cid, case):
        if case.path not in ("julia_bla", "juliax_bla"):
            return False
        v, r = dc.view_of(case), dc.restated(case)
        b = dc.bailout_of(case)
        try:
            if case.path == "julia_bla":
                P, Q = J.reference_orbits(v, b)
                got, counts = JB.restate_bla(v, case.W, case.H, 1, b, orbits=(P, Q), tabs=JB.bla_tables(P, Q)[::-1])
            else:
                Px, Qx = J.reference_orbits_x(v, b)
                got, counts = JB.restate_x_bla(v, case.W, case.H, 1, b, orbits=(Px, Qx), tabs=JB.bla_tables_x(Px, Qx)[::-1])
        except IndexError:
            return True                                               # a lane looked past the end of the other orbit's table
        by_counts = tuple(int(c) for c in counts) != r.counts
        print(cid, "counts", tuple(counts), "for", r.counts, "iter differing", int((got[0][0] != r.samples[0][0]).sum()))
        return by_counts
    bad = _failing(dc.GROUPS_BY_ID["short"] + dc.GROUPS_BY_ID["small"], fails)
    # every flagged Julia small case sees it by its counts (at bailout 0.75 P's lanes take no BLA step at all); the short
    # frames do not: a shallow delta is above every radius of either table, and the counts of both builds are the plain steps
    assert sorted(bad) == sorted(cid for cid in dc.GROUPS_BY_ID["small"] if dc.CASES[cid].path in ("julia_bla", "juliax_bla"))
    assert "small/julia_bla-RABBIT30-b0.75" in bad and "small/juliax_bla-RABBIT30-b0.75" in bad
    assert not {dc.CASES[cid].path for cid in bad} & set(dc.OLD_PATHS)


def test_wrong_build_8_the_de_blocks_shade_or_edge_dropped(oracle):
    """DeepDePart of a block with shade left 0 (rgba is fr_render_deep's), or with edge_px left 0 (de / 0: the smoothstep
    saturates and nothing is shaded either): every shaded colour case fails.  The old table rendered no DE kernel."""
    shaded = [cid for cid in dc.GROUPS_BY_ID["colour"] if dc.CASES[cid].params.get("shade")]
    assert len(shaded) == 32

    def no_shade(cid, case):
        return _rgb_fails(dc.expected_rgb(oracle, case, dict(case.params, shade=False)), dc.expected_rgb(oracle, case))

    def no_edge(cid, case):
        with np.errstate(all="ignore"):
            got = dc.expected_rgb(oracle, case, dict(case.params, edge_px=0.0))
        return _rgb_fails(got, dc.expected_rgb(oracle, case))
    assert _failing(shaded, no_shade) == shaded
    assert _failing(shaded, no_edge) == shaded
    assert not {dc.CASES[cid].path for cid in shaded} & set(dc.OLD_PATHS)
