"""What tests/test_deep_ship_de_gpu.py (fr_render_deep_ship_de) and tests/test_deepx_ship_de_gpu.py (fr_render_deepx_ship_de) share:
the renders through Renderer.render_deep_ship_de and the plain ship calls, the expectations from tests/deep_ship_de_ref.py, and
the checks themselves, each taking ext = False (fp64 deltas, the zoom from the state) or True (extended deltas, the zoom string
of the view)."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_de_ref as DE
import deep_ship_de_ref as SD
import deep_ship_ref as S
import deepx_ship_ref as XS

DE_TOL = 2.0 ** -50          # relative: only the device log is not correctly rounded (test_deepx_de_gpu's bound)
RGB_TOL = 1e-4               # test_deep_ship_gpu's
NAMES = ("rgba", "nu", "iter", "de", "deriv")

# the views by name, and the edges: max_iterations 1, 2, 3 on the shallow view, whose frame has escapes from the second update on
# (at max_iterations 1 every pixel is interior)
VIEWS = dict(SD.views())
VIEWS.update({"n%d" % n: dict(S.SHALLOW, max_iter=n) for n in (1, 2, 3)})


def few(bad, n):
    """palette wrap exceptions (test_deep_ship_gpu._few)"""
    return int(bad.sum()) <= max(2, int(0.001 * n))


def view_of(name, ext):
    v = VIEWS[name]
    if ext and not isinstance(v["zoom"], str):
        return XS.as_x_view(v)
    assert ext or not isinstance(v["zoom"], str), name
    return v


@functools.lru_cache(maxsize=None)
def restated(name, w, h, ext, aa=1, bla=False):
    """computed once per case, shared, never changed: (samples, counts); a sample is (iter, r2, J, [Je,] z)"""
    v = view_of(name, ext)
    return SD.restate_x_de(v, w, h, aa, bla=bla) if ext else SD.restate_de(v, w, h, aa, bla=bla)


def planes_of(v, smp, ext):
    """(iter, de, deriv) of a restated sample"""
    if ext:
        it, r2, J, Je, z = smp
        return it, SD.de_x_of(it, r2, J, Je, z, v["max_iter"]), SD.deriv_x_of(it, J, Je, v["max_iter"])
    it, r2, J, z = smp
    return it, SD.de_of(it, r2, J, z, v["max_iter"]), SD.deriv_of(it, J, v["max_iter"])


def state(fr, v, ext, aa=1, bailout=4.0):
    if ext:
        return fr.FractalState(max_iterations=v["max_iter"], antialiasing_samples=aa, bailout=bailout)
    return fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"], antialiasing_samples=aa, bailout=bailout)


def deep_view(fr, v, ext):
    return fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"]) if ext else fr.DeepView(v["cx"], v["cy"])


def host_planes(rows, w, names=NAMES):
    shapes = dict(rgba=((rows, w, 4), np.float32), nu=((rows, w), np.float64), iter=((rows, w), np.int32),
                  de=((rows, w), np.float64), deriv=((rows, w, 4), np.float64))
    return {k: np.empty(*shapes[k]) for k in names}


def render_de(fr, r, v, w, h, ext, aa=1, post=False, bla=False, shade=False, edge=1.8, shard=None, bailout=4.0):
    out = host_planes(shard.rows(h) if shard else h, w)
    r.render_deep_ship_de(state(fr, v, ext, aa, bailout), w, h, deep_view(fr, v, ext), post_chain=post, shade=shade, edge_px=edge,
                          shard=shard, bla=bla, **out)
    return out


def plain_call(r, ext):
    return r.render_deepx_ship if ext else r.render_deep_ship


def render_plain_entry(fr, r, v, w, h, ext, aa=1, post=False, bla=False, bailout=4.0):
    """fr_render_deep_ship / fr_render_deepx_ship with the same parameters"""
    out = host_planes(h, w, NAMES[:3])
    plain_call(r, ext)(state(fr, v, ext, aa, bailout), w, h, deep_view(fr, v, ext), post_chain=post, bla=bla, **out)
    return out


def steps(r, ext):
    return tuple(r.last_deepx_ship_steps() if ext else r.last_deep_ship_steps())


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def check_de(de, ref):
    zero = ref == 0.0
    assert np.all(de[zero] == 0.0)
    with np.errstate(all="ignore"):
        rel = np.abs(de[~zero] - ref[~zero]) / np.abs(ref[~zero])
    fin = np.isfinite(ref[~zero])
    assert np.array_equal(de[~zero][~fin].view(np.uint64), ref[~zero][~fin].view(np.uint64))
    worst = float(rel[fin].max()) if fin.any() else 0.0
    print(f"worst |de - restated| / |restated| = {worst:.3g} (2^-50 = {DE_TOL:.3g})")
    assert worst <= DE_TOL, worst


def check_case(fr, r, name, w, h, aa, bla, ext):
    """deriv and iter bit for bit the restatement's, de within 2^-50 relative and exactly 0 where the restatement's is; rgba
    (shade 0), nu, iter and the step counts byte for byte those of the plain ship entry point with the same parameters"""
    v = view_of(name, ext)
    samples, counts = restated(name, w, h, ext, aa, bla)
    it, ref_de, ref_deriv = planes_of(v, samples[0], ext)
    got = render_de(fr, r, v, w, h, ext, aa, bla=bla)
    st = steps(r, ext) if bla else None
    assert np.array_equal(got["iter"], it), int((got["iter"] != it).sum())
    assert same_bytes(got["deriv"], ref_deriv), int((got["deriv"] != ref_deriv).sum())
    check_de(got["de"], ref_de)
    interior = it == v["max_iter"]
    assert np.all(got["de"][interior] == 0.0) and not got["deriv"][interior].any()
    if bla:
        assert st == tuple(counts), (st, counts)
    base = render_plain_entry(fr, r, v, w, h, ext, aa, bla=bla)
    for k in NAMES[:3]:
        assert same_bytes(got[k], base[k]), k
    if bla:
        assert steps(r, ext) == st
    return v, samples, counts, got


def expected_shaded(oracle, v, samples, w, h, aa, post, edge, ext):
    """the colour stage of test_deep_ship_gpu with the shading on every escaped sub-sample, before the average"""
    p = oracle.OracleParams(fractal=2, max_iterations=v["max_iter"], zoom=1.0, aa=aa, post_chain=0)
    acc = np.zeros((h, w, 3), np.float32)
    for smp in samples:
        it, de, _ = planes_of(v, smp, ext)
        rgb = oracle.colorize(p, S.smooth(it, smp[1], v["max_iter"]))[..., :3]
        acc = acc + DE.shade(rgb, de, it < v["max_iter"], edge)
    if aa > 1:
        acc = acc / np.float32(aa * aa)
    if post:
        acc = np.array([oracle.post_chain(c, julia_floors=1) for c in acc.reshape(-1, 3)], np.float32).reshape(h, w, 3)
    return acc


def check_shading(fr, r, oracle, name, w, h, aa, edge, post, bla, ext):
    v = view_of(name, ext)
    samples, _ = restated(name, w, h, ext, aa, bla)
    got = render_de(fr, r, v, w, h, ext, aa, post=post, bla=bla, shade=True, edge=edge)
    assert np.all(got["rgba"][..., 3] == 1.0)
    want = expected_shaded(oracle, v, samples, w, h, aa, post, edge, ext)
    bad = np.abs(got["rgba"][..., :3] - want).max(axis=2) > RGB_TOL
    assert few(bad, w * h), int(bad.sum())
    flat = render_de(fr, r, v, w, h, ext, aa, post=post, bla=bla)
    assert (got["rgba"] != flat["rgba"]).any(axis=2).sum() >= 1
    assert np.all(got["rgba"][..., :3] <= flat["rgba"][..., :3]) or post      # the shading only darkens a linear colour
    for k in ("nu", "iter", "de", "deriv"):
        assert same_bytes(got[k], flat[k]), k


def check_plumbing(fr, r, name, bla, ext):
    """shards of 5 and 7 rows: the five planes of each part equal the matching rows of the whole frame byte for byte (s comes
    from the whole frame), packed into host and device planes and in place under FR_LAYOUT_FRAME; the asynchronous form on a
    caller's stream; any single plane of the five alone"""
    import torch
    v = view_of(name, ext)
    w, h, aa = 48, 36, 2
    ref = render_de(fr, r, v, w, h, ext, aa, post=True, bla=bla, shade=True)
    ref_steps = steps(r, ext) if bla else None
    assert (ref["iter"] < v["max_iter"]).any() and ref["deriv"].any()
    dev = torch.device("cuda:0")

    def planes(rows, fill=0):
        t = dict(rgba=torch.full((rows, w, 4), fill, dtype=torch.float32, device=dev),
                 nu=torch.full((rows, w), fill, dtype=torch.float64, device=dev),
                 iter=torch.full((rows, w), -7, dtype=torch.int32, device=dev),
                 de=torch.full((rows, w), fill, dtype=torch.float64, device=dev),
                 deriv=torch.full((rows, w, 4), fill, dtype=torch.float64, device=dev))
        torch.cuda.synchronize()
        return t

    st = state(fr, v, ext, aa)
    view = deep_view(fr, v, ext)
    kw = dict(post_chain=True, shade=True, bla=bla)
    F = fr._capi
    L = fr.lib()
    p = st.to_params(fr.FractalType.BurningShip, fr.Precision.F64, True)
    if bla:
        p.flags |= F.FR_FLAG_DEEPX_SHIP_BLA if ext else F.FR_FLAG_DEEP_SHIP_BLA
    cv = view.to_cx() if ext else view.to_c()
    entry = L.fr_render_deepx_ship_de if ext else L.fr_render_deep_ship_de
    for strip in (5, 7):
        tot = np.zeros(3, np.int64)
        for part in range(3):
            sh = fr.Shard(part, 3, strip)
            g = sh.global_rows(h)
            assert len(g)
            host = render_de(fr, r, v, w, h, ext, aa, post=True, bla=bla, shade=True, shard=sh)          # FR_MEM_HOST, packed
            if bla:
                tot += np.array(steps(r, ext))
            d = planes(len(g))
            r.render_deep_ship_de(st, w, h, view, shard=sh, **kw, **d)                                    # FR_MEM_DEVICE, packed
            for k in NAMES:
                assert same_bytes(host[k], ref[k][g]), (strip, part, k)
                assert same_bytes(d[k].cpu().numpy(), ref[k][g]), (strip, part, k)
        if bla:
            assert tuple(tot) == ref_steps
        # FR_LAYOUT_FRAME: each part writes its rows in place into whole-frame device planes, deriv four doubles per pixel
        d = planes(h)
        o = F.fr_output(d["rgba"].data_ptr(), d["nu"].data_ptr(), d["iter"].data_ptr(), F.FR_MEM_DEVICE, F.FR_LAYOUT_FRAME)
        e = F.fr_deep_de(d["de"].data_ptr(), d["deriv"].data_ptr(), 1, 1.8)
        for part in (1, 0, 2):
            sh = F.fr_shard(part, 3, strip)
            assert entry(r._ctx, C.byref(p), C.byref(cv), C.byref(e), w, h, C.byref(sh), C.byref(o)) == 0
        for k in NAMES:
            assert same_bytes(d[k].cpu().numpy(), ref[k]), (strip, k)
    # host planes cannot be written in place
    host_o = F.fr_output(None, None, None, F.FR_MEM_HOST, F.FR_LAYOUT_FRAME)
    he = F.fr_deep_de(np.zeros((h, w)).ctypes.data, None, 0, 1.8)
    assert entry(r._ctx, C.byref(p), C.byref(cv), C.byref(he), w, h, None, C.byref(host_o)) == F.FR_ERR_INVALID_ARG
    # the asynchronous form on a caller's stream
    d = planes(h)
    s = torch.cuda.Stream()
    r.render_deep_ship_de(st, w, h, view, stream=s.cuda_stream, sync=False, **kw, **d)
    s.synchronize()
    r.check()
    for k in NAMES:
        assert same_bytes(d[k].cpu().numpy(), ref[k]), k
    if bla:
        assert steps(r, ext) == ref_steps
    with pytest.raises(fr.FractalRendererError):                                  # host planes: the synchronous form only
        r.render_deep_ship_de(st, w, h, view, de=np.empty((h, w)), sync=False, bla=bla)
    # any single plane of the five alone, host and device
    for k in NAMES:
        alone = host_planes(h, w, (k,))
        r.render_deep_ship_de(st, w, h, view, **kw, **alone)
        assert same_bytes(alone[k], ref[k]), k
    only = torch.full((h, w, 4), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    r.render_deep_ship_de(st, w, h, view, deriv=only, **kw)
    assert same_bytes(only.cpu().numpy(), ref["deriv"])
    with pytest.raises(fr.FractalRendererError):                                  # no plane at all
        r.render_deep_ship_de(st, w, h, view, bla=bla)


def check_shared_state(fr, name, ext):
    """After the plain ship entry point (flagged) of a view, the distance call builds no table -- whose key holds the orbit
    slot's generation, so no orbit was computed or uploaded either -- and the reverse; the step counts are one slot's.  Then
    the orbit cache key: a distance call at another bailout behind a plain call gives the bytes of the same call on a fresh
    context, and so does the plain call behind it."""
    v = view_of(name, ext)
    w, h = 32, 24
    L = fr.lib()
    mine = (3 if ext else 0) + 1                                    # fr_deep_bla_builds(extended, formula): the ship is formula 1

    def builds(r):
        return [int(L.fr_deep_bla_builds(r._ctx, x, f)) for x in (0, 1) for f in (0, 1, 2)]

    def want(n):
        b = [0] * 6
        b[mine] = n
        return b

    it = np.empty((h, w), np.int32)
    for de_first in (False, True):
        with fr.Renderer(0) as r:
            st, view = state(fr, v, ext), deep_view(fr, v, ext)
            de = np.empty((h, w), np.float64)

            def one(which, bla):
                if which:
                    r.render_deep_ship_de(st, w, h, view, de=de, bla=bla)
                else:
                    plain_call(r, ext)(st, w, h, view, bla=bla, iter=it)

            assert builds(r) == [0] * 6
            one(de_first, True)
            assert builds(r) == want(1)
            st1 = steps(r, ext)
            one(not de_first, True)
            assert builds(r) == want(1) and steps(r, ext) == st1
            one(de_first, False)                                  # unflagged renders in between keep the table
            one(not de_first, False)
            one(de_first, True)
            assert builds(r) == want(1) and steps(r, ext) == st1
            for other in ((r.last_deep_ship_steps, r.last_deepx_steps) if ext else (r.last_deepx_ship_steps, r.last_deep_steps)):
                with pytest.raises(fr.FractalRendererError):
                    other()
    with fr.Renderer(0) as r:
        alone_de = render_de(fr, r, v, w, h, ext, bla=True, bailout=2.0)
    with fr.Renderer(0) as r:
        alone_plain = render_plain_entry(fr, r, v, w, h, ext, bla=True, bailout=4.0)
    with fr.Renderer(0) as r:
        render_plain_entry(fr, r, v, w, h, ext, bla=True, bailout=4.0)
        got = render_de(fr, r, v, w, h, ext, bla=True, bailout=2.0)
        for k in NAMES:
            assert same_bytes(got[k], alone_de[k]), k
        back = render_plain_entry(fr, r, v, w, h, ext, bla=True, bailout=4.0)
        for k in NAMES[:3]:
            assert same_bytes(back[k], alone_plain[k]), k
        assert builds(r) == want(3)                                # each change of the bailout is a new orbit and a new table
