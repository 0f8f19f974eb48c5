"""Deep views with bilinear approximation (FR_FLAG_DEEP_BLA): the parts that need no GPU -- the restatement against the
plain perturbation step, the table's properties, how much it skips, view C, and the ABI."""
import os
import re

import numpy as np

import deep_bla_ref as BR
import deep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 256, 192


def _orbit(v):
    return R.reference_orbit(v["cx"], v["cy"], v["zoom"], v["max_iter"])


def _updates(it, max_iter):
    """the updates the plain step executes: i + 1 for a sample that escaped at i, max_iter otherwise"""
    it = it.astype(np.int64)
    return int(np.where(it < max_iter, it + 1, max_iter).sum())


def test_without_radius_it_is_the_plain_step():
    """eps = 0: every r is 0, no BLA step is taken and the planes are deep_ref.perturb's, bit for bit"""
    for v in (R.VIEW_A, R.VIEW_B):
        orb = _orbit(v)
        samples, counts = BR.restate_bla(v, W, H, orbit=orb, eps=0.0)
        (it, r2), = samples
        pit, pr2, _ = R.perturb(orb, *R.sample_dc(W, H, v["zoom"], 1, 0), v["max_iter"])
        assert counts[1] == 0 and counts[2] == 0
        assert counts[0] == _updates(pit, v["max_iter"])
        assert np.array_equal(it, pit) and np.array_equal(r2.view(np.uint64), pr2.view(np.uint64))


def test_table_radius_is_monotone_in_the_level():
    for v in (R.VIEW_A, R.VIEW_B, BR.VIEW_C):
        orb = _orbit(v)
        tab = BR.bla_table(orb, BR.dcmax(W, H, v["zoom"]))
        N = len(orb) - 1
        assert len(tab) == BR.levels(N) == (N - 1).bit_length() - 1
        single = BR.EPS * np.sqrt(orb[1:N, 0] * orb[1:N, 0] + orb[1:N, 1] * orb[1:N, 1])
        prev = single
        for k, T in enumerate(tab, 1):
            assert len(T["r"]) == (N - 1) >> k
            assert np.all(T["r"] >= 0.0) and np.all(T["r"] <= prev[0:2 * len(T["r"]):2])
            prev = T["r"]
        assert any(np.any(T["r"] > 0.0) for T in tab)


def test_table_radius_is_zero_where_it_must_be():
    # c = -2: Z_m = 2 from m = 2 on, |A| of 2^k steps is 4^(2^k): level 9 and up overflow, and their r is 0
    orb = R.reference_orbit("-2", "0", 1e-20, 3000)
    assert len(orb) - 1 == 3000
    tab = BR.bla_table(orb, BR.dcmax(W, H, 1e-20))
    nonfinite = 0
    for T in tab:
        bad = ~(np.isfinite(T["ax"]) & np.isfinite(T["ay"]) & np.isfinite(T["bx"]) & np.isfinite(T["by"]))
        nonfinite += int(bad.sum())
        assert np.all(T["r"][bad] == 0.0)
    assert nonfinite > 0
    # centre 0: every Z_m = 0, so every single step has r = 0 and so has every level (|A_x| = 0 included)
    orb = R.reference_orbit("0", "0", 1e-20, 500)
    assert len(orb) - 1 == 500 and not orb.any()
    tab = BR.bla_table(orb, BR.dcmax(W, H, 1e-20))
    assert len(tab) == 8 and all(np.all(T["r"] == 0.0) for T in tab)
    samples, counts = BR.restate_bla(dict(cx="0", cy="0", zoom=1e-20, max_iter=500), 64, 48, orbit=orb)
    assert counts[1] == 0 and np.all(samples[0][0] == 500)


def test_bla_skips_on_the_deep_views():
    """The share of trips (plain + BLA steps) in the plain-only updates, from the restatement at 256 x 192, aa 1:
    B 0.173 and C 0.069 (A 0.56, the shallow view 1.0: it takes no BLA step, its |dc| is far above every radius).
    The bars leave room for neither to regress by much: B <= 0.20, C <= 0.10."""
    for v, bar in ((R.VIEW_B, 0.20), (BR.VIEW_C, 0.10)):
        orb = _orbit(v)
        samples, counts = BR.restate_bla(v, W, H, orbit=orb)
        (it, _), = samples
        plain_only = _updates(R.perturb(orb, *R.sample_dc(W, H, v["zoom"], 1, 0), v["max_iter"])[0], v["max_iter"])
        assert counts[0] + counts[2] == _updates(it, v["max_iter"])     # every update is a plain step or skipped
        assert counts[1] > 0 and (counts[0] + counts[1]) <= bar * plain_only, (counts, plain_only)
    _, counts = BR.restate_bla(R.SHALLOW, W, H)
    assert counts[1] == 0


def test_view_c_sits_next_to_a_minibrot():
    v = BR.VIEW_C
    assert v["zoom"] <= 1e-50 and 5000 <= v["max_iter"] <= 50000
    orb = _orbit(v)
    assert len(orb) - 1 == v["max_iter"]                                    # the reference is interior
    it, _, _ = R.perturb(orb, *R.sample_dc(W, H, v["zoom"], 1, 0), v["max_iter"])
    assert (it < v["max_iter"]).mean() >= 0.30 and (it == v["max_iter"]).mean() >= 0.10
    # the escape counts spread over the frame: no single value covers a large share of the escaped samples
    esc = it[it < v["max_iter"]]
    assert np.unique(esc, return_counts=True)[1].max() <= 0.05 * esc.size


def test_flag_and_counts_are_in_the_header_and_capi(fr):
    hdr = open(os.path.join(ROOT, "include", "fractalrenderer_amd.h")).read()
    assert re.search(r"#define FR_FLAG_DEEP_BLA\s+0x2u", hdr)
    assert re.search(r"#define FR_HAS_DEEP_BLA 1", hdr)
    assert re.search(r"int fr_ctx_last_deep_steps\(fr_ctx\* ctx, uint64_t out\[3\]\);", hdr)
    assert fr._capi.FR_FLAG_DEEP_BLA == 0x2 == fr.FR_FLAG_DEEP_BLA
    assert "fr_ctx_last_deep_steps" in fr._capi.SIGNATURES
    assert hasattr(fr.lib(), "fr_ctx_last_deep_steps")
    assert fr.DeepSteps(1, 2, 3).skipped == 3
    import inspect
    assert inspect.signature(fr.Renderer.render_deep).parameters["bla"].default is False
