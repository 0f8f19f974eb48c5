"""Deep Julia views with extended-exponent deltas on the GPU (fr_render_deepx_julia): byte identity with fr_render_deep_julia
where a double holds the view (the flush and the plain-to-extended switch on superattracting interior pixels included),
the planes against the extended restatement at 1e-400 and 1e-1000, the exact iteration there, and the zoom string's rules."""
import numpy as np
import pytest

import deep_julia_ref as J

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4
NU_TOL = 1e-9


def _few(bad, n):
    return int(bad.sum()) <= max(2, int(0.001 * n))


def _state(fr, v, aa=1, zoom=None):
    return fr.FractalState(zoom=v["zoom"] if zoom is None else zoom, max_iterations=v["max_iter"], antialiasing_samples=aa,
                           julia_c_real=v["c"][0], julia_c_imag=v["c"][1])


def _render(fr, r, v, w, h, aa=1, post=False, zoom_s=None, extended=True):
    rgba = np.empty((h, w, 4), np.float32)
    nu = np.empty((h, w), np.float64)
    it = np.empty((h, w), np.int32)
    if extended:       # state.zoom is not read there: give it one no view of the tests has
        r.render_deep_julia(_state(fr, v, aa, zoom=2.5), w, h, fr.DeepView(v["cx"], v["cy"], zoom=zoom_s or v["zoom_s"]),
                            post_chain=post, rgba=rgba, nu=nu, iter=it)
    else:
        r.render_deep_julia(_state(fr, v, aa), w, h, fr.DeepView(v["cx"], v["cy"]), post_chain=post, rgba=rgba, nu=nu, iter=it)
    return rgba, nu, it


def _same(got, want):
    return all(np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)) for g, w in zip(got, want))


@pytest.mark.parametrize("aa,post", [(1, False), (2, True)])
@pytest.mark.parametrize("name", ["RABBIT30", "DENDRITE100", "BASILICA30"])
def test_bytes_of_the_fp64_entry_point_where_a_double_holds_the_view(fr, renderer, name, aa, post):
    v = J.view(name)
    w, h = 256, 192
    want = _render(fr, renderer, v, w, h, aa, post, extended=False)
    got = _render(fr, renderer, v, w, h, aa, post)
    print(name, "iter differing", int((got[2] != want[2]).sum()), "interior", float((want[2] == v["max_iter"]).mean()))
    assert _same(got, want)
    if name == "BASILICA30":       # the view of the flush: its interior is there, and the restatement's flush fires on it
        assert (want[2] == v["max_iter"]).mean() >= 0.5
        stats = {}
        assert np.array_equal(J.restate_x(v, 64, 48, stats=stats)[0][0], _render(fr, renderer, v, 64, 48)[2])
        assert stats["flushes"] > 0


def test_a_zoom_string_a_double_holds_gives_the_fp64_bytes(fr, renderer):
    v = dict(J.SHALLOW[3])
    for zs, z in (("1.0", 1.0), ("0.2", 0.2), ("1e-13", 1e-13), ("3e-290", 3e-290)):
        v["zoom"], v["zoom_s"] = z, zs
        assert _same(_render(fr, renderer, v, 64, 48, 2, True), _render(fr, renderer, v, 64, 48, 2, True, extended=False)), zs


@pytest.mark.parametrize("aa,post", [(1, False), (2, True)])
@pytest.mark.parametrize("name", ["DENDRITE400", "DENDRITE1000"])
def test_planes_match_the_extended_restatement(fr, renderer, oracle, name, aa, post):
    v = J.view(name)
    w, h = J.XW, J.XH
    rgba, nu, it = _render(fr, renderer, v, w, h, aa, post)
    samples, stats = J.restated_x(name, aa)
    r_it, r_r2 = samples[0]
    print(name, aa, post, stats, "iter mismatches", int((it != r_it).sum()), "range", r_it.min(), r_it.max())
    assert stats["ext_steps"] > stats["plain_steps"]
    assert np.array_equal(it, r_it), int((it != r_it).sum())
    dnu = np.abs(nu - J.smooth(r_it, r_r2, v["max_iter"])).max()
    print("max |dnu|", dnu)
    assert dnu <= NU_TOL
    assert np.all(rgba[..., 3] == 1.0)
    p = oracle.OracleParams(fractal=1, max_iterations=v["max_iter"], aa=aa, post_chain=0)
    acc = np.zeros((h, w, 3), np.float32)
    for s_it, s_r2 in samples:
        acc = acc + oracle.colorize(p, J.smooth(s_it, s_r2, v["max_iter"]))[..., :3]
    if aa > 1:
        acc = acc / np.float32(aa * aa)
    if post:
        acc = np.array([oracle.post_chain(c, julia_floors=1) for c in acc.reshape(-1, 3)], np.float32).reshape(h, w, 3)
    bad = np.abs(rgba[..., :3] - acc).max(axis=2) > RGB_TOL
    assert _few(bad, w * h), int(bad.sum())


@pytest.mark.parametrize("name", ["DENDRITE400", "DENDRITE1000"])
def test_extended_views_are_exact(fr, renderer, name):
    v = J.view(name)
    _, _, it = _render(fr, renderer, v, J.XW, J.XH)
    ex = J.exact_samples_x(name)
    ys, xs = J.random_pixels(J.XW, J.XH)
    largest = np.unique(ex, return_counts=True)[1].max() / len(ex)
    agreement = (it[ys, xs] == ex).mean()
    print(name, "exact", ex.min(), ex.max(), "largest class", largest, "agreement", agreement)
    assert largest <= 0.80
    assert agreement >= 0.99


def test_zoom_strings_are_validated(fr, renderer):
    v = J.view("DENDRITE30")
    out = np.empty((36, 48), np.int32)
    for z in ("1e-1001", "2e3", "z", "", "0", "-1"):
        with pytest.raises(fr._capi.FractalRendererError) as e:
            renderer.render_deep_julia(_state(fr, v), 48, 36, fr.DeepView(v["cx"], v["cy"], zoom=z), iter=out)
        assert e.value.status == fr._capi.FR_ERR_INVALID_ARG, z
    for z in ("1e-1000", "1e3"):
        renderer.render_deep_julia(_state(fr, J.SHALLOW[0]), 48, 36, fr.DeepView("0", "0", zoom=z), iter=out)
