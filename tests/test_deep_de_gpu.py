"""Distance estimates for deep Mandelbrot views on the GPU (fr_render_deep_de): the five planes against the numpy
restatement (tests/deep_de_ref.py) and against fr_render_deep, plain and with FR_FLAG_DEEP_BLA; the shading; shards, layouts,
memory kinds, the asynchronous form; and the caches it shares with fr_render_deep."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_bla_ref as BR
import deep_de_ref as D
import deep_ref as R
from test_deep_gpu import RGB_TOL, _few      # the rgba tolerance of test_deep_gpu.test_planes_match_the_restatement

pytestmark = pytest.mark.gpu

DE_TOL = 2.0 ** -50          # relative: the device log and numpy's are each within 1 ulp, two roundings follow them
VIEWS = {"shallow": R.SHALLOW, "A": R.VIEW_A, "B": R.VIEW_B, "C": BR.VIEW_C, "tip": D.TIP}


def _view(name, max_iter=None):
    v = VIEWS[name]
    return v if max_iter is None else dict(v, max_iter=max_iter)


def _state(fr, v, aa=1, bailout=4.0):
    return fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"], antialiasing_samples=aa, bailout=bailout)


@functools.lru_cache(maxsize=None)
def _restated(name, w, h, aa=1, bla=False, bailout=4.0, max_iter=None):
    """computed once per case, shared, never changed"""
    return D.restate_de(_view(name, max_iter), w, h, aa, bailout, bla=bla)


def _render_de(fr, r, v, w, h, aa=1, post=False, bla=False, shade=False, edge=1.8, shard=None, bailout=4.0):
    rows = shard.rows(h) if shard else h
    out = dict(rgba=np.empty((rows, w, 4), np.float32), nu=np.empty((rows, w), np.float64), iter=np.empty((rows, w), np.int32),
               de=np.empty((rows, w), np.float64), deriv=np.empty((rows, w, 2), np.float64))
    r.render_deep_de(_state(fr, v, aa, bailout), w, h, fr.DeepView(v["cx"], v["cy"]), post_chain=post, shade=shade, edge_px=edge,
                     shard=shard, bla=bla, **out)
    return out


def _render_plain_entry(fr, r, v, w, h, aa=1, post=False, bla=False, bailout=4.0):
    """fr_render_deep with the same parameters"""
    out = dict(rgba=np.empty((h, w, 4), np.float32), nu=np.empty((h, w), np.float64), iter=np.empty((h, w), np.int32))
    r.render_deep(_state(fr, v, aa, bailout), w, h, fr.DeepView(v["cx"], v["cy"]), post_chain=post, bla=bla, **out)
    return out


def _same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _check_de(de, ref):
    zero = ref == 0.0
    assert np.all(de[zero] == 0.0)
    with np.errstate(all="ignore"):
        rel = np.abs(de[~zero] - ref[~zero]) / np.abs(ref[~zero])
    fin = np.isfinite(ref[~zero])
    assert np.array_equal(de[~zero][~fin].view(np.uint64), ref[~zero][~fin].view(np.uint64))
    worst = float(rel[fin].max()) if fin.any() else 0.0
    print(f"worst |de - restated| / |restated| = {worst:.3g} (2^-50 = {DE_TOL:.3g})")
    assert worst <= DE_TOL, worst


CASES = [("A", 48, 36, 1, 4.0, None), ("A", 48, 36, 2, 4.0, None), ("C", 32, 24, 1, 4.0, None), ("tip", 21, 13, 1, 4.0, None),
         ("shallow", 40, 24, 1, 0.75, None), ("A", 48, 36, 1, 4.0, 1), ("A", 48, 36, 1, 4.0, 2), ("A", 48, 36, 1, 4.0, 3),
         ("A", 48, 36, 1, 0.5, 1), ("A", 48, 36, 1, 0.5, 3)]


@pytest.mark.parametrize("bla", [False, True], ids=["plain", "bla"])
@pytest.mark.parametrize("name,w,h,aa,bailout,max_iter", CASES,
                         ids=["%s-%dx%d-aa%d-b%g-n%s" % c for c in CASES])
def test_planes_match_the_restatement_and_fr_render_deep(fr, renderer, name, w, h, aa, bailout, max_iter, bla):
    """deriv and iter bit for bit the restatement's, de within 2^-50 relative and exactly 0 where the restatement's is; rgba
    (shade 0), nu, iter and the step counts byte for byte those of fr_render_deep with the same parameters.
    A's reference escapes (rebases at m == N); C rebases once per period and takes levels up to 12; the tip is the bottom of
    the range on a ragged frame; the shallow view at bailout 0.75 has log|z| < 0 and takes no BLA step; max_iter 1 .. 3 clip
    the level (u + 2^k <= max_iter), and at bailout 0.5 every sample escapes in the first update, with D = (s, 0) exactly."""
    v = _view(name, max_iter)
    samples, counts = _restated(name, w, h, aa, bla, bailout, max_iter)
    it, r2, Dx, Dy = samples[0]
    got = _render_de(fr, renderer, v, w, h, aa, bla=bla, bailout=bailout)
    steps = tuple(renderer.last_deep_steps()) if bla else None
    assert np.array_equal(got["iter"], it), int((got["iter"] != it).sum())
    assert _same_bytes(got["deriv"], D.deriv_of(it, Dx, Dy, v["max_iter"]))
    ref_de = D.de_of(it, r2, Dx, Dy, v["max_iter"])
    _check_de(got["de"], ref_de)
    assert np.all(got["de"][it == v["max_iter"]] == 0.0) and not got["deriv"][it == v["max_iter"]].any()
    if bla:
        assert steps == tuple(counts), (steps, counts)
    base = _render_plain_entry(fr, renderer, v, w, h, aa, bla=bla, bailout=bailout)
    for k in ("rgba", "nu", "iter"):
        assert _same_bytes(got[k], base[k]), k
    if bla:
        assert tuple(renderer.last_deep_steps()) == steps
    # what each case is there for
    esc = it < v["max_iter"]
    if name == "shallow":
        assert (ref_de[esc] < 0.0).any() and counts[1] == 0
    elif name == "C" and bla:
        assert counts[1] > 0 and counts[2] > 10 * counts[0]
    elif name == "tip":
        assert esc.any() and float(D.spacing(v["zoom"], h)) < 1e-290
    if bailout == 0.5:
        assert esc.all() and np.all(got["iter"] == 0)
        assert np.all(got["deriv"][..., 0] == D.spacing(v["zoom"], h)) and not got["deriv"][..., 1].any()


@pytest.mark.parametrize("bla", [False, True], ids=["plain", "bla"])
def test_byte_identity_with_fr_render_deep(fr, renderer, bla):
    """aa 2 with the post chain on a ragged frame: rgba at shade 0, nu, iter and fr_ctx_last_deep_steps"""
    v, w, h = R.VIEW_B, 61, 45
    got = _render_de(fr, renderer, v, w, h, 2, post=True, bla=bla)
    steps = tuple(renderer.last_deep_steps()) if bla else None
    base = _render_plain_entry(fr, renderer, v, w, h, 2, post=True, bla=bla)
    for k in ("rgba", "nu", "iter"):
        assert _same_bytes(got[k], base[k]), k
    if bla:
        assert steps == tuple(renderer.last_deep_steps()) and steps[1] > 0


def _expected_shaded(oracle, v, samples, w, h, aa, post, edge):
    """the colour stage of test_deep_gpu._expected_rgba with the shading on every escaped sub-sample, before the average"""
    p = oracle.OracleParams(max_iterations=v["max_iter"], zoom=v["zoom"], aa=aa, post_chain=0)
    acc = np.zeros((h, w, 3), np.float32)
    for it, r2, Dx, Dy in samples:
        rgb = oracle.colorize(p, R.smooth(it, r2, v["max_iter"]))[..., :3]
        acc = acc + D.shade(rgb, D.de_of(it, r2, Dx, Dy, v["max_iter"]), it < v["max_iter"], edge)
    if aa > 1:
        acc = acc / np.float32(aa * aa)
    if post:
        acc = np.array([oracle.post_chain(c) for c in acc.reshape(-1, 3)], np.float32).reshape(h, w, 3)
    return acc


@pytest.mark.parametrize("bla", [False, True], ids=["plain", "bla"])
@pytest.mark.parametrize("post", [False, True], ids=["linear", "post"])
@pytest.mark.parametrize("edge", [1.8, 0.25])
def test_shading(fr, renderer, oracle, edge, post, bla):
    v, w, h, aa = R.VIEW_A, 48, 36, 2
    samples, _ = _restated("A", w, h, aa, bla)
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
    form on a caller's stream; a call with nothing but de"""
    import torch
    v, w, h, aa = R.VIEW_A, 48, 36, 2
    names = ("rgba", "nu", "iter", "de", "deriv")
    ref = _render_de(fr, renderer, v, w, h, aa, post=True, bla=bla, shade=True)
    ref_steps = tuple(renderer.last_deep_steps()) if bla else None
    dev = torch.device("cuda:0")

    def planes(rows, fill=0):
        t = dict(rgba=torch.full((rows, w, 4), fill, dtype=torch.float32, device=dev),
                 nu=torch.full((rows, w), fill, dtype=torch.float64, device=dev),
                 iter=torch.full((rows, w), -7, dtype=torch.int32, device=dev),
                 de=torch.full((rows, w), fill, dtype=torch.float64, device=dev),
                 deriv=torch.full((rows, w, 2), fill, dtype=torch.float64, device=dev))
        torch.cuda.synchronize()
        return t

    st = _state(fr, v, aa)
    view = fr.DeepView(v["cx"], v["cy"])
    kw = dict(post_chain=True, shade=True, bla=bla)
    tot = np.zeros(3, np.int64)
    for part in range(3):
        sh = fr.Shard(part, 3, 8)
        g = sh.global_rows(h)
        assert len(g)
        host = _render_de(fr, renderer, v, w, h, aa, post=True, bla=bla, shade=True, shard=sh)       # FR_MEM_HOST, packed
        if bla:
            tot += np.array(renderer.last_deep_steps())
        d = planes(len(g))
        renderer.render_deep_de(st, w, h, view, shard=sh, **kw, **d)                                   # FR_MEM_DEVICE, packed
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
        p.flags |= fr.FR_FLAG_DEEP_BLA
    cv = view.to_c()
    d = planes(h)
    o = F.fr_output(d["rgba"].data_ptr(), d["nu"].data_ptr(), d["iter"].data_ptr(), F.FR_MEM_DEVICE, F.FR_LAYOUT_FRAME)
    e = F.fr_deep_de(d["de"].data_ptr(), d["deriv"].data_ptr(), 1, 1.8)
    for part in (1, 0, 2):
        sh = F.fr_shard(part, 3, 8)
        assert L.fr_render_deep_de(renderer._ctx, C.byref(p), C.byref(cv), C.byref(e), w, h, C.byref(sh), C.byref(o)) == 0
    for k in names:
        assert _same_bytes(d[k].cpu().numpy(), ref[k]), k
    # host planes cannot be written in place
    host_o = F.fr_output(None, None, None, F.FR_MEM_HOST, F.FR_LAYOUT_FRAME)
    he = F.fr_deep_de(np.zeros((h, w)).ctypes.data, None, 0, 1.8)
    assert L.fr_render_deep_de(renderer._ctx, C.byref(p), C.byref(cv), C.byref(he), w, h, None, C.byref(host_o)) == F.FR_ERR_INVALID_ARG
    # the asynchronous form on a caller's stream
    d = planes(h)
    s = torch.cuda.Stream()
    renderer.render_deep_de(st, w, h, view, stream=s.cuda_stream, sync=False, **kw, **d)
    s.synchronize()
    renderer.check()
    for k in names:
        assert _same_bytes(d[k].cpu().numpy(), ref[k]), k
    if bla:
        assert tuple(renderer.last_deep_steps()) == ref_steps
    with pytest.raises(fr.FractalRendererError):                                  # host planes: the synchronous form only
        renderer.render_deep_de(st, w, h, view, de=np.empty((h, w)), sync=False, bla=bla)
    # nothing but de
    for de in (np.full((h, w), -1.0), torch.full((h, w), -1.0, dtype=torch.float64, device=dev)):
        torch.cuda.synchronize()
        renderer.render_deep_de(st, w, h, view, de=de, bla=bla)
        assert _same_bytes(de if isinstance(de, np.ndarray) else de.cpu().numpy(), ref["de"])
    only = np.full((h, w, 2), -1.0)
    renderer.render_deep_de(st, w, h, view, deriv=only, bla=bla)
    assert _same_bytes(only, ref["deriv"])
    with pytest.raises(fr.FractalRendererError):                                  # no plane at all
        renderer.render_deep_de(st, w, h, view, bla=bla)


def test_caches_are_fr_render_deeps_own(fr):
    """After fr_render_deep(BLA) of a view, fr_render_deep_de(BLA) of it builds no table -- whose key holds the orbit slot's
    generation, so no orbit was uploaded either -- and the reverse; the ship's and Julia's slots and the extended ones are
    never touched."""
    v, w, h = R.VIEW_B, 48, 36
    L = fr.lib()

    def builds(r):
        return [int(L.fr_deep_bla_builds(r._ctx, x, f)) for x in (0, 1) for f in (0, 1, 2)]

    plain = dict(iter=np.empty((h, w), np.int32))
    for de_first in (False, True):
        with fr.Renderer(0) as r:
            st, view = _state(fr, v), fr.DeepView(v["cx"], v["cy"])
            de = np.empty((h, w), np.float64)

            def one(which, bla):
                if which:
                    r.render_deep_de(st, w, h, view, de=de, bla=bla)
                else:
                    r.render_deep(st, w, h, view, bla=bla, **plain)

            assert builds(r) == [0] * 6
            one(de_first, True)
            assert builds(r) == [1, 0, 0, 0, 0, 0]
            steps = tuple(r.last_deep_steps())
            one(not de_first, True)
            assert builds(r) == [1, 0, 0, 0, 0, 0] and tuple(r.last_deep_steps()) == steps
            one(de_first, False)                                  # unflagged renders in between keep the table
            one(not de_first, False)
            one(de_first, True)
            assert builds(r) == [1, 0, 0, 0, 0, 0] and tuple(r.last_deep_steps()) == steps
            r.render_deep_de(_state(fr, dict(v, zoom=2e-100)), w, h, view, de=de, bla=True)   # another dcmax: a rebuild, as there
            assert builds(r) == [2, 0, 0, 0, 0, 0]
            for other in (r.last_deep_ship_steps, r.last_deep_julia_steps, r.last_deepx_steps):
                with pytest.raises(fr.FractalRendererError):
                    other()
