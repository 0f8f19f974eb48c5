"""What tests/test_deep_julia_de_gpu.py (fr_render_deep_julia_de) and tests/test_deepx_julia_de_gpu.py (fr_render_deepx_julia_de)
share: the renders through Renderer.render_deep_julia_de and render_deep_julia, the expectations from tests/deep_julia_de_ref.py,
and the checks themselves, each taking ext = False (fp64 deltas, the zoom from the state) or True (extended deltas, the zoom
string of the view)."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_cases as DC
import deep_julia_de_ref as JD
import deep_julia_ref as J
import deepx_ref as X

DE_TOL = 2.0 ** -50          # relative: the device log and numpy's are each within 1 ulp (test_deep_de_gpu.DE_TOL)
RGB_TOL = 1e-4               # test_deep_julia_gpu.RGB_TOL
NAMES = ("rgba", "nu", "iter", "de", "deriv")


def few(bad, n):
    """palette wrap exceptions (test_deep_julia_gpu._few)"""
    return int(bad.sum()) <= max(2, int(0.001 * n))


def for_x(v):
    """a view as the extended entry point resolves it: the automatic F of its zoom string"""
    return dict(v, F=X.frac_bits_x(v["zoom_s"]))


# The edges, (view, bailout): max_iterations 1, 2, 3 on deep_cases.J_N3, whose frame splits into 2, 3 and 4 iter classes there (up
# to 2 neither orbit has a table: the flagged kernel without one); the c = -1 basin at max_iterations 64 (the flush of D); a primary
# orbit of 1, 2 and 3 updates (deep_cases.J_N1 .. J_N3, with their max_iterations); an escape at update 0 -- the centre inside
# bailout 1.25 and P_1 outside, so that D = 2 z_0 s, one product; bailout 0.75 (log|z| < 0, N_Q = 2, a third of the samples
# leave P) and 65536.
ESC0 = dict(name="ESC0", c=(0.0, 1.0), cx="1.2", cy="0.25", zoom=0.05, zoom_s="0.05", max_iter=16, F=J.R.frac_bits(0.05))
EDGES = {"n1": (dict(DC.J_N3, max_iter=1), 4.0), "n2": (dict(DC.J_N3, max_iter=2), 4.0), "n3": (dict(DC.J_N3, max_iter=3), 4.0),
         "np1": (DC.J_N1, 4.0), "np2": (DC.J_N2, 4.0), "np3": (DC.J_N3, 4.0), "esc0": (ESC0, 1.25),
         "b0.75": (J.view("RABBIT30"), 0.75), "b65536": (J.view("DENDRITE30"), 65536.0),
         "basin": (JD.basin_view((-1.0, 0.0)), 4.0)}
SHORT_NP = {"np1": 1, "np2": 2, "np3": 3}


def view_of(name, ext):
    v, bailout = EDGES[name] if name in EDGES else (JD.view(name), 4.0)
    return (for_x(v) if ext and name in EDGES else v), bailout


@functools.lru_cache(maxsize=None)
def restated(name, w, h, ext, aa=1, bla=False):
    """computed once per case, shared, never changed: (samples, counts); a sample is (iter, r2, Dx, Dy[, eD])"""
    v, bailout = view_of(name, ext)
    if name not in EDGES:
        return (JD.restated_x if ext else JD.restated)(name, w, h, aa, bla)
    return (JD.restate_x_de if ext else JD.restate_de)(v, w, h, aa, bailout, bla=bla)


def planes_of(v, smp, ext):
    """(iter, de, deriv) of a restated sample"""
    if ext:
        it, r2, Dx, Dy, eD = smp
        return it, JD.de_of_x(it, r2, Dx, Dy, eD, v["max_iter"]), JD.deriv_of_x(it, Dx, Dy, eD, v["max_iter"])
    it, r2, Dx, Dy = smp
    return it, JD.de_of(it, r2, Dx, Dy, v["max_iter"]), JD.deriv_of(it, Dx, Dy, v["max_iter"])


def state(fr, v, aa=1, bailout=4.0):
    return fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"], antialiasing_samples=aa, bailout=bailout,
                           julia_c_real=v["c"][0], julia_c_imag=v["c"][1])


def deep_view(fr, v, ext):
    return fr.DeepView(v["cx"], v["cy"], zoom=v["zoom_s"]) if ext else fr.DeepView(v["cx"], v["cy"])


def host_planes(rows, w, names=NAMES):
    shapes = dict(rgba=((rows, w, 4), np.float32), nu=((rows, w), np.float64), iter=((rows, w), np.int32),
                  de=((rows, w), np.float64), deriv=((rows, w, 2), np.float64))
    return {k: np.empty(*shapes[k]) for k in names}


def render_de(fr, r, v, w, h, ext, aa=1, post=False, bla=False, shade=False, edge=1.8, shard=None, bailout=4.0):
    out = host_planes(shard.rows(h) if shard else h, w)
    r.render_deep_julia_de(state(fr, v, aa, bailout), w, h, deep_view(fr, v, ext), post_chain=post, shade=shade, edge_px=edge,
                           shard=shard, bla=bla, **out)
    return out


def render_plain_entry(fr, r, v, w, h, ext, aa=1, post=False, bla=False, bailout=4.0):
    """fr_render_deep_julia / fr_render_deepx_julia with the same parameters"""
    out = host_planes(h, w, NAMES[:3])
    r.render_deep_julia(state(fr, v, aa, bailout), w, h, deep_view(fr, v, ext), post_chain=post, bla=bla, **out)
    return out


def steps(r, ext):
    return tuple(r.last_deepx_julia_steps() if ext else r.last_deep_julia_steps())


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
    (shade 0), nu, iter and the step counts byte for byte those of the plain Julia entry point with the same parameters"""
    v, bailout = view_of(name, ext)
    samples, counts = restated(name, w, h, ext, aa, bla)
    it, ref_de, ref_deriv = planes_of(v, samples[0], ext)
    got = render_de(fr, r, v, w, h, ext, aa, bla=bla, bailout=bailout)
    st = steps(r, ext) if bla else None
    assert np.array_equal(got["iter"], it), int((got["iter"] != it).sum())
    assert same_bytes(got["deriv"], ref_deriv)
    check_de(got["de"], ref_de)
    interior = it == v["max_iter"]
    assert np.all(got["de"][interior] == 0.0) and not got["deriv"][interior].any()
    if bla:
        assert st == tuple(counts), (st, counts)
    base = render_plain_entry(fr, r, v, w, h, ext, aa, bla=bla, bailout=bailout)
    for k in NAMES[:3]:
        assert same_bytes(got[k], base[k]), k
    if bla:
        assert steps(r, ext) == st
    return v, bailout, samples, counts, got


def check_edge(fr, r, name, bla, ext):
    w, h = 32, 24
    v, bailout, samples, counts, got = check_case(fr, r, name, w, h, 1, bla, ext)
    it = samples[0][0]
    esc = it < v["max_iter"]
    # what each case is there for
    P, Q = J.reference_orbits(v, bailout)
    if name in ("n1", "n2", "n3"):
        assert len(np.unique(it)) == v["max_iter"] + 1
    if name in ("n1", "n2"):
        assert counts[1] == 0 and len(P) - 1 <= 2 and len(Q) - 1 <= 2      # no table for either orbit: N <= 2
    if name == "basin":                                            # the flush on the device: zero D inside, a live one outside
        assert esc.any() and not esc.all() and np.all(np.isfinite(got["de"][esc])) and np.all(got["de"][esc] > 0.0)
    if name in SHORT_NP:
        assert len(P) - 1 == SHORT_NP[name]
    if name == "esc0":                                             # D = 2 z_0 s by hand, from the planes alone
        assert len(P) - 1 == 1 and np.all(got["iter"] == 0)
        mx, my = J.S.sample_dc(w, h, v["zoom"], 1, 0)
        s = JD.spacing(v["zoom"], h)
        zx, zy = np.float64(float(v["cx"])) + mx, np.float64(float(v["cy"])) + my
        assert same_bytes(got["deriv"][..., 0], (zx + zx) * s) and same_bytes(got["deriv"][..., 1], (zy + zy) * s)
    if name == "b0.75":
        assert (got["de"][esc] < 0.0).any() and len(Q) - 1 == 2
    if name == "b65536":
        assert esc.all() and float(np.sqrt(samples[0][1].max())) > 65536.0


def expected_shaded(oracle, v, samples, w, h, aa, post, edge, ext):
    """the colour stage of test_deep_julia_gpu._expected_rgba with the shading on every escaped sub-sample, before the average"""
    p = oracle.OracleParams(fractal=1, max_iterations=v["max_iter"], zoom=v["zoom"], aa=aa, post_chain=0)
    acc = np.zeros((h, w, 3), np.float32)
    for smp in samples:
        it, de, _ = planes_of(v, smp, ext)
        rgb = oracle.colorize(p, J.smooth(it, smp[1], v["max_iter"]))[..., :3]
        acc = acc + JD.shade(rgb, de, it < v["max_iter"], edge)
    if aa > 1:
        acc = acc / np.float32(aa * aa)
    if post:
        acc = np.array([oracle.post_chain(c, julia_floors=1) for c in acc.reshape(-1, 3)], np.float32).reshape(h, w, 3)
    return acc


def check_shading(fr, r, oracle, name, w, h, aa, edge, post, bla, ext):
    v, _ = view_of(name, ext)
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
    v, _ = view_of(name, ext)
    w, h, aa = 48, 36, 2
    ref = render_de(fr, r, v, w, h, ext, aa, post=True, bla=bla, shade=True)
    ref_steps = steps(r, ext) if bla else None
    dev = torch.device("cuda:0")

    def planes(rows, fill=0):
        t = dict(rgba=torch.full((rows, w, 4), fill, dtype=torch.float32, device=dev),
                 nu=torch.full((rows, w), fill, dtype=torch.float64, device=dev),
                 iter=torch.full((rows, w), -7, dtype=torch.int32, device=dev),
                 de=torch.full((rows, w), fill, dtype=torch.float64, device=dev),
                 deriv=torch.full((rows, w, 2), fill, dtype=torch.float64, device=dev))
        torch.cuda.synchronize()
        return t

    st = state(fr, v, aa)
    view = deep_view(fr, v, ext)
    kw = dict(post_chain=True, shade=True, bla=bla)
    F = fr._capi
    L = fr.lib()
    p = st.to_params(fr.FractalType.JuliaSet, fr.Precision.F64, True)
    if bla:
        p.flags |= fr.FR_FLAG_DEEPX_JULIA_BLA if ext else fr.FR_FLAG_DEEP_JULIA_BLA
    cv = view.to_cx() if ext else view.to_c()
    entry = L.fr_render_deepx_julia_de if ext else L.fr_render_deep_julia_de
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
            r.render_deep_julia_de(st, w, h, view, shard=sh, **kw, **d)                                   # FR_MEM_DEVICE, packed
            for k in NAMES:
                assert same_bytes(host[k], ref[k][g]), (strip, part, k)
                assert same_bytes(d[k].cpu().numpy(), ref[k][g]), (strip, part, k)
        if bla:
            assert tuple(tot) == ref_steps
        # FR_LAYOUT_FRAME: each part writes its rows in place into whole-frame device planes
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
    r.render_deep_julia_de(st, w, h, view, stream=s.cuda_stream, sync=False, **kw, **d)
    s.synchronize()
    r.check()
    for k in NAMES:
        assert same_bytes(d[k].cpu().numpy(), ref[k]), k
    if bla:
        assert steps(r, ext) == ref_steps
    with pytest.raises(fr.FractalRendererError):                                  # host planes: the synchronous form only
        r.render_deep_julia_de(st, w, h, view, de=np.empty((h, w)), sync=False, bla=bla)
    # any single plane of the five alone, host and device
    for k in NAMES:
        alone = host_planes(h, w, (k,))
        r.render_deep_julia_de(st, w, h, view, **kw, **alone)
        assert same_bytes(alone[k], ref[k]), k
    only = torch.full((h, w), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    r.render_deep_julia_de(st, w, h, view, de=only, **kw)
    assert same_bytes(only.cpu().numpy(), ref["de"])
    with pytest.raises(fr.FractalRendererError):                                  # no plane at all
        r.render_deep_julia_de(st, w, h, view, bla=bla)


def check_shared_state(fr, name, ext):
    """After the plain Julia entry point (flagged) of a view, the distance call builds no table -- whose key holds the orbit
    slot's generation, so no orbit was uploaded either -- and the reverse; the Mandelbrot and ship slots survive it all."""
    v, _ = view_of(name, ext)
    w, h = 32, 24
    L = fr.lib()
    mine = (3 if ext else 0) + 2                                    # fr_deep_bla_builds(extended, formula): Julia is formula 2

    def builds(r):
        return [int(L.fr_deep_bla_builds(r._ctx, x, f)) for x in (0, 1) for f in (0, 1, 2)]

    def want(n, others):
        b = list(others)
        b[mine] = n
        return b

    mv, sv = DC.VIEWS["A"], DC.VIEWS["SHIP_A"]
    it = np.empty((h, w), np.int32)
    for de_first in (False, True):
        with fr.Renderer(0) as r:
            st, view = state(fr, v), deep_view(fr, v, ext)
            de = np.empty((h, w), np.float64)

            def others():
                r.render_deep(fr.FractalState(zoom=mv["zoom"], max_iterations=mv["max_iter"]), w, h, fr.DeepView(mv["cx"], mv["cy"]),
                              bla=True, iter=it)
                r.render_deep_ship(fr.FractalState(zoom=sv["zoom"], max_iterations=sv["max_iter"]), w, h,
                                   fr.DeepView(sv["cx"], sv["cy"]), bla=True, iter=it)
                return tuple(r.last_deep_steps()), tuple(r.last_deep_ship_steps())

            def one(which, bla):
                if which:
                    r.render_deep_julia_de(st, w, h, view, de=de, bla=bla)
                else:
                    r.render_deep_julia(st, w, h, view, bla=bla, iter=it)

            assert builds(r) == [0] * 6
            other_steps = others()
            base = builds(r)
            assert base == [1, 1, 0, 0, 0, 0]
            one(de_first, True)
            assert builds(r) == want(1, base)
            st1 = steps(r, ext)
            one(not de_first, True)
            assert builds(r) == want(1, base) and steps(r, ext) == st1
            one(de_first, False)                                  # unflagged renders in between keep the table
            one(not de_first, False)
            one(de_first, True)
            assert builds(r) == want(1, base) and steps(r, ext) == st1
            assert others() == other_steps                        # the Mandelbrot and ship orbits and tables are still there
            assert builds(r) == want(1, base)
            for other in ((r.last_deep_julia_steps, r.last_deepx_steps) if ext else (r.last_deepx_julia_steps, r.last_deepx_steps)):
                with pytest.raises(fr.FractalRendererError):
                    other()
