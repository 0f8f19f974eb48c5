"""Distance estimates for extended views on the GPU (fr_render_deepx_de): the five planes against the numpy restatement
(tests/deepx_de_ref.py) and against fr_render_deepx, plain and with FR_FLAG_DEEPX_BLA; shallow views against fr_render_deep_de;
the shading; shards, layouts, memory kinds, the asynchronous form; and the caches it shares with fr_render_deepx."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_ref as R
import deepx_de_ref as XD
import deepx_ref as X
from test_deep_de_gpu import DE_TOL, _check_de, _same_bytes      # 2^-50 relative, zeros and non-finite values exactly
from test_deep_gpu import RGB_TOL, _few

pytestmark = pytest.mark.gpu

V = dict(X.views(), tip400=dict(cx="-2", cy="0", zoom="1e-400", max_iter=1400),
         A=dict(R.VIEW_A, zoom="1e-30"), B=dict(R.VIEW_B, zoom="1e-100"))


def _state(fr, v, aa=1):
    return fr.FractalState(max_iterations=v["max_iter"], antialiasing_samples=aa)


def _xv(fr, v):
    return fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"])


@functools.lru_cache(maxsize=None)
def _orbit(name):
    return X.orbit_of(V[name])


@functools.lru_cache(maxsize=None)
def _restated(name, w, h, aa=1, bla=False):
    """computed once per case, shared, never changed"""
    return XD.restate_x_de(V[name], w, h, aa, bla=bla, orbit=_orbit(name))


def _render_de(fr, r, v, w, h, aa=1, post=False, bla=False, shade=False, edge=1.8, shard=None):
    rows = shard.rows(h) if shard else h
    out = dict(rgba=np.empty((rows, w, 4), np.float32), nu=np.empty((rows, w), np.float64), iter=np.empty((rows, w), np.int32),
               de=np.empty((rows, w), np.float64), deriv=np.empty((rows, w, 2), np.float64))
    r.render_deepx_de(_state(fr, v, aa), w, h, _xv(fr, v), post_chain=post, shade=shade, edge_px=edge, shard=shard, bla=bla, **out)
    return out


def _render_deepx(fr, r, v, w, h, aa=1, post=False, bla=False):
    """fr_render_deepx with the same parameters"""
    out = dict(rgba=np.empty((h, w, 4), np.float32), nu=np.empty((h, w), np.float64), iter=np.empty((h, w), np.int32))
    r.render_deep(_state(fr, v, aa), w, h, _xv(fr, v), post_chain=post, xbla=bla, **out)
    return out


CASES = [("D", 48, 36, 1), ("D", 24, 18, 2), ("T130", 48, 36, 1), ("T300", 32, 24, 1), ("E", 32, 24, 1), ("tip400", 21, 13, 1)]


@pytest.mark.parametrize("bla", [False, True], ids=["plain", "bla"])
@pytest.mark.parametrize("name,w,h,aa", CASES, ids=["%s-%dx%d-aa%d" % c for c in CASES])
def test_planes_match_the_restatement_and_fr_render_deepx(fr, renderer, name, w, h, aa, bla):
    """deriv and iter bit for bit the restatement's (every operation on D is a correctly rounded IEEE operation or an exact
    scaling), de within 2^-50 relative and exactly 0 where the restatement's is; rgba (shade 0), nu, iter and the step counts
    byte for byte those of fr_render_deepx with the same parameters.  D and E stay extended for most of the orbit; T130 starts
    extended and turns plain; T300 sits at the edge of the double range; the tip is a ragged frame whose every sample escapes."""
    v = V[name]
    samples, counts = _restated(name, w, h, aa, bla)
    it, r2, Dx, Dy, eD = samples[0]
    got = _render_de(fr, renderer, v, w, h, aa, bla=bla)
    steps = tuple(renderer.last_deepx_steps()) if bla else None
    assert np.array_equal(got["iter"], it), int((got["iter"] != it).sum())
    assert _same_bytes(got["deriv"], XD.deriv_of_x(it, Dx, Dy, eD, v["max_iter"]))
    ref_de = XD.de_of_x(it, r2, Dx, Dy, eD, v["max_iter"])
    _check_de(got["de"], ref_de)
    esc = it < v["max_iter"]
    assert esc.sum() >= 50 and np.all(np.isfinite(got["de"])) and np.all(got["de"][esc] > 0.0)
    assert np.all(got["de"][~esc] == 0.0) and not got["deriv"][~esc].any()
    if bla:
        assert steps == tuple(counts) and counts[1] > 0, (steps, counts)
    base = _render_deepx(fr, renderer, v, w, h, aa, bla=bla)
    for k in ("rgba", "nu", "iter"):
        assert _same_bytes(got[k], base[k]), k
    if bla:
        assert tuple(renderer.last_deepx_steps()) == steps
    if name == "tip400":
        assert esc.all()


@pytest.mark.parametrize("name", ["A", "B"])
def test_shallow_views_are_fr_render_deep_des_byte_for_byte(fr, renderer, name):
    """VIEW_A and VIEW_B as extended views, plain: de and deriv (and rgba, nu, iter) are fr_render_deep_de's bytes -- the
    extended D is the fp64 D with its exponent held apart"""
    v, w, h = V[name], 48, 36
    got = _render_de(fr, renderer, v, w, h, post=True)
    want = dict(rgba=np.empty((h, w, 4), np.float32), nu=np.empty((h, w), np.float64), iter=np.empty((h, w), np.int32),
                de=np.empty((h, w), np.float64), deriv=np.empty((h, w, 2), np.float64))
    renderer.render_deep_de(fr.FractalState(zoom=float(v["zoom"]), max_iterations=v["max_iter"]), w, h,
                            fr.DeepView(v["cx"], v["cy"]), post_chain=True, **want)
    assert (want["iter"] < v["max_iter"]).sum() >= 100 and want["de"].any()
    for k in ("de", "deriv", "rgba", "nu", "iter"):
        assert _same_bytes(got[k], want[k]), k


def _expected_shaded(oracle, v, samples, w, h, aa, post, edge):
    """the colour stage of test_deepx_gpu._expected_rgba with the shading on every escaped sub-sample, before the average"""
    p = oracle.OracleParams(max_iterations=v["max_iter"], zoom=1.0, aa=aa, post_chain=0)
    acc = np.zeros((h, w, 3), np.float32)
    for it, r2, Dx, Dy, eD in samples:
        rgb = oracle.colorize(p, R.smooth(it, r2, v["max_iter"]))[..., :3]
        acc = acc + XD.shade(rgb, XD.de_of_x(it, r2, Dx, Dy, eD, v["max_iter"]), it < v["max_iter"], edge)
    if aa > 1:
        acc = acc / np.float32(aa * aa)
    if post:
        acc = np.array([oracle.post_chain(c) for c in acc.reshape(-1, 3)], np.float32).reshape(h, w, 3)
    return acc


@pytest.mark.parametrize("bla", [False, True], ids=["plain", "bla"])
@pytest.mark.parametrize("post", [False, True], ids=["linear", "post"])
@pytest.mark.parametrize("edge", [1.8, 0.25])
def test_shading(fr, renderer, oracle, edge, post, bla):
    name, w, h, aa = "D", 24, 18, 2
    v = V[name]
    samples, _ = _restated(name, w, h, aa, bla)
    got = _render_de(fr, renderer, v, w, h, aa, post=post, bla=bla, shade=True, edge=edge)
    assert np.all(got["rgba"][..., 3] == 1.0)
    want = _expected_shaded(oracle, v, samples, w, h, aa, post, edge)
    bad = np.abs(got["rgba"][..., :3] - want).max(axis=2) > RGB_TOL
    assert _few(bad, w * h), int(bad.sum())
    flat = _render_de(fr, renderer, v, w, h, aa, post=post, bla=bla)
    assert (got["rgba"] != flat["rgba"]).any(axis=2).sum() >= 1
    assert np.all(got["rgba"][..., :3] <= flat["rgba"][..., :3]) or post      # the shading only darkens a linear colour
    for k in ("nu", "iter", "de", "deriv"):
        assert _same_bytes(got[k], flat[k]), k


@pytest.mark.parametrize("bla", [False, True], ids=["plain", "bla"])
def test_shards_layouts_memory_and_async(fr, renderer, bla):
    """three parts of 8-row strips: the five planes of each part equal the matching rows of the whole frame byte for byte (s and
    dcmax come from the whole frame), packed into host and device planes and in place under FR_LAYOUT_FRAME; the asynchronous
    form on a caller's stream; calls with nothing but de, nothing but deriv, and no plane at all"""
    import torch
    v, w, h, aa = V["D"], 24, 18, 2
    names = ("rgba", "nu", "iter", "de", "deriv")
    ref = _render_de(fr, renderer, v, w, h, aa, post=True, bla=bla, shade=True)
    ref_steps = tuple(renderer.last_deepx_steps()) if bla else None
    dev = torch.device("cuda:0")

    def planes(rows, fill=0):
        t = dict(rgba=torch.full((rows, w, 4), fill, dtype=torch.float32, device=dev),
                 nu=torch.full((rows, w), fill, dtype=torch.float64, device=dev),
                 iter=torch.full((rows, w), -7, dtype=torch.int32, device=dev),
                 de=torch.full((rows, w), fill, dtype=torch.float64, device=dev),
                 deriv=torch.full((rows, w, 2), fill, dtype=torch.float64, device=dev))
        torch.cuda.synchronize()
        return t

    st, view = _state(fr, v, aa), _xv(fr, v)
    kw = dict(post_chain=True, shade=True, bla=bla)
    tot = np.zeros(3, np.int64)
    for part in range(3):
        sh = fr.Shard(part, 3, 8)
        g = sh.global_rows(h)
        assert len(g)
        host = _render_de(fr, renderer, v, w, h, aa, post=True, bla=bla, shade=True, shard=sh)       # FR_MEM_HOST, packed
        if bla:
            tot += np.array(renderer.last_deepx_steps())
        d = planes(len(g))
        renderer.render_deepx_de(st, w, h, view, shard=sh, **kw, **d)                                  # FR_MEM_DEVICE, packed
        for k in names:
            assert _same_bytes(host[k], ref[k][g]), (part, k)
            assert _same_bytes(d[k].cpu().numpy(), ref[k][g]), (part, k)
    if bla:
        assert tuple(tot) == ref_steps
    # FR_LAYOUT_FRAME: each part writes its rows in place into whole-frame device planes
    F = fr._capi
    L = fr.lib()
    p = st.to_params(fr.FractalType.Mandelbrot, fr.Precision.F64, True)
    if bla:
        p.flags |= fr.FR_FLAG_DEEPX_BLA
    cv = view.to_cx()
    d = planes(h)
    o = F.fr_output(d["rgba"].data_ptr(), d["nu"].data_ptr(), d["iter"].data_ptr(), F.FR_MEM_DEVICE, F.FR_LAYOUT_FRAME)
    e = F.fr_deep_de(d["de"].data_ptr(), d["deriv"].data_ptr(), 1, 1.8)
    for part in (1, 0, 2):
        sh = F.fr_shard(part, 3, 8)
        assert L.fr_render_deepx_de(renderer._ctx, C.byref(p), C.byref(cv), C.byref(e), w, h, C.byref(sh), C.byref(o)) == 0
    for k in names:
        assert _same_bytes(d[k].cpu().numpy(), ref[k]), k
    # host planes cannot be written in place
    host_o = F.fr_output(None, None, None, F.FR_MEM_HOST, F.FR_LAYOUT_FRAME)
    he = F.fr_deep_de(np.zeros((h, w)).ctypes.data, None, 0, 1.8)
    assert L.fr_render_deepx_de(renderer._ctx, C.byref(p), C.byref(cv), C.byref(he), w, h, None, C.byref(host_o)) == F.FR_ERR_INVALID_ARG
    # the asynchronous form on a caller's stream
    d = planes(h)
    s = torch.cuda.Stream()
    renderer.render_deepx_de(st, w, h, view, stream=s.cuda_stream, sync=False, **kw, **d)
    s.synchronize()
    renderer.check()
    for k in names:
        assert _same_bytes(d[k].cpu().numpy(), ref[k]), k
    if bla:
        assert tuple(renderer.last_deepx_steps()) == ref_steps
    with pytest.raises(fr.FractalRendererError):                                  # host planes: the synchronous form only
        renderer.render_deepx_de(st, w, h, view, de=np.empty((h, w)), sync=False, bla=bla)
    # rgba NULL: nothing but de
    for de in (np.full((h, w), -1.0), torch.full((h, w), -1.0, dtype=torch.float64, device=dev)):
        torch.cuda.synchronize()
        renderer.render_deepx_de(st, w, h, view, de=de, bla=bla)
        assert _same_bytes(de if isinstance(de, np.ndarray) else de.cpu().numpy(), ref["de"])
    only = np.full((h, w, 2), -1.0)
    renderer.render_deepx_de(st, w, h, view, deriv=only, bla=bla)
    assert _same_bytes(only, ref["deriv"])
    with pytest.raises(fr.FractalRendererError):                                  # no plane at all
        renderer.render_deepx_de(st, w, h, view, bla=bla)


def test_caches_are_fr_render_deepxs_own(fr):
    """After fr_render_deepx(BLA) of a view, fr_render_deepx_de(BLA) of it builds no table -- whose key holds the orbit slot's
    generation, so no orbit was computed either -- and the reverse; fr_ctx_last_deepx_steps is the one both write; the fp64
    slots and the other formulas' are never touched."""
    v, w, h = V["T130"], 32, 24
    L = fr.lib()

    def builds(r):
        return [int(L.fr_deep_bla_builds(r._ctx, x, f)) for x in (0, 1) for f in (0, 1, 2)]

    plain = dict(iter=np.empty((h, w), np.int32))
    for de_first in (False, True):
        with fr.Renderer(0) as r:
            st, view = _state(fr, v), _xv(fr, v)
            de = np.empty((h, w), np.float64)

            def one(which, bla):
                if which:
                    r.render_deepx_de(st, w, h, view, de=de, bla=bla)
                else:
                    r.render_deep(st, w, h, view, xbla=bla, **plain)

            assert builds(r) == [0] * 6
            one(de_first, True)
            assert builds(r) == [0, 0, 0, 1, 0, 0]
            steps = tuple(r.last_deepx_steps())
            one(not de_first, True)
            assert builds(r) == [0, 0, 0, 1, 0, 0] and tuple(r.last_deepx_steps()) == steps
            one(de_first, False)                                  # unflagged renders in between keep the table
            one(not de_first, False)
            one(de_first, True)
            assert builds(r) == [0, 0, 0, 1, 0, 0] and tuple(r.last_deepx_steps()) == steps
            r.render_deepx_de(st, w, h, fr.DeepView(v["cx"], v["cy"], zoom="2e-130"), de=de, bla=True)   # another dcmax: a rebuild
            assert builds(r) == [0, 0, 0, 2, 0, 0]
            for other in (r.last_deep_steps, r.last_deep_ship_steps, r.last_deep_julia_steps, r.last_deepx_ship_steps):
                with pytest.raises(fr.FractalRendererError):
                    other()
