"""Phoenix on the GPU (fr_render_phoenix): against the executed shader, the numpy restatement at realistic sizes, shards,
the asynchronous form, Julia mode, and its coexistence with the other kernels on one context."""
import ctypes as C

import numpy as np
import pytest

import phoenix_ref
from test_phoenix_host import params_of, phx, ref_kwargs   # noqa: F401  (phx: the fixture)

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4          # after the post chain; the linear plane is held to the same bar
NU_TOL_F64 = 1e-9


def _few(bad, n):
    """palette wrap exceptions: a sample whose t sits on a knot or on fract's wrap may take the neighbouring colour"""
    return int(bad.sum()) <= max(2, int(0.001 * n))


def _ulp_ok(nu, ref):
    ulp = np.spacing(np.maximum(np.abs(ref), 1.0).astype(np.float32)).astype(np.float64)
    return np.abs(nu.astype(np.float64) - ref.astype(np.float64)) <= 4 * ulp + 4e-6


def _render(fr, r, st, ph, W, H, precision, post=False, shard=None):
    rows = shard.rows(H) if shard else H
    rgba = np.empty((rows, W, 4), np.float32)
    nu = np.empty((rows, W), np.float64 if precision == fr.Precision.F64 else np.float32)
    it = np.empty((rows, W), np.int32)
    r.render_phoenix(st, W, H, ph, precision=precision, post_chain=post, rgba=rgba, nu=nu, iter=it, shard=shard)
    return rgba, nu, it


def test_fixture_cases_fp32(fr, renderer, phx):   # noqa: F811
    for name, (W, H, p, rgba_ref, it_ref, sm_ref) in phx.items():
        st, ph = params_of(fr, p)
        rgba, nu, it = _render(fr, renderer, st, ph, W, H, fr.Precision.F32, post=True)
        assert not np.isnan(rgba).any(), name
        assert np.all(rgba[..., 3] == 1.0)
        bad = np.abs(rgba[..., :3] - rgba_ref[..., :3]).max(axis=2) > RGB_TOL
        assert _few(bad, W * H), (name, int(bad.sum()))
        if it_ref is not None:
            assert np.array_equal(it, it_ref), name
            assert np.all(_ulp_ok(nu, sm_ref)), name
        lin, nu2, it2 = _render(fr, renderer, st, ph, W, H, fr.Precision.F32, post=False)
        r_it, r_sm, r_rgb = phoenix_ref.render(W, H, **ref_kwargs(p))
        assert np.array_equal(it2, r_it) and np.all(_ulp_ok(nu2, r_sm)), name
        bad = np.abs(lin[..., :3] - r_rgb).max(axis=2) > RGB_TOL
        assert _few(bad, W * H), (name, int(bad.sum()))


@pytest.mark.parametrize("W,H,max_iter", [(1700, 900, 256), (1024, 768, 1024)])
@pytest.mark.parametrize("f64", [False, True])
def test_realistic_sizes_against_the_restatement(fr, renderer, W, H, max_iter, f64):
    st = fr.FractalState(max_iterations=max_iter)
    prec = fr.Precision.F64 if f64 else fr.Precision.F32
    rgba, nu, it = _render(fr, renderer, st, fr.PhoenixParams(), W, H, prec)
    r_it, r_sm, r_rgb = phoenix_ref.render(W, H, max_iterations=max_iter, f64=f64)
    assert np.array_equal(it, r_it)
    if f64:
        assert np.abs(nu - r_sm).max() <= NU_TOL_F64
    else:
        assert np.all(_ulp_ok(nu, r_sm))
    bad = np.abs(rgba[..., :3] - r_rgb).max(axis=2) > RGB_TOL
    assert _few(bad, W * H), int(bad.sum())


@pytest.mark.parametrize("f64", [False, True])
def test_row_bands_of_a_4096_frame(fr, renderer, f64):
    import torch
    W = H = 4096
    prec = fr.Precision.F64 if f64 else fr.Precision.F32
    dev = torch.device("cuda:0")
    it = torch.empty((H, W), dtype=torch.int32, device=dev)
    nu = torch.empty((H, W), dtype=torch.float64 if f64 else torch.float32, device=dev)
    rgba = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    renderer.render_phoenix(fr.FractalState(max_iterations=1024), W, H, precision=prec, rgba=rgba, nu=nu, iter=it)
    for r0 in (0, 1500, 2044, 4080):
        rows = np.arange(r0, r0 + 16)
        r_it, r_sm, r_rgb = phoenix_ref.render(W, H, max_iterations=1024, f64=f64, rows=rows)
        g_it, g_nu, g_rgb = it[r0:r0 + 16].cpu().numpy(), nu[r0:r0 + 16].cpu().numpy(), rgba[r0:r0 + 16].cpu().numpy()
        assert np.array_equal(g_it, r_it), r0
        assert (np.abs(g_nu - r_sm).max() <= NU_TOL_F64) if f64 else np.all(_ulp_ok(g_nu, r_sm)), r0
        assert _few(np.abs(g_rgb[..., :3] - r_rgb).max(axis=2) > RGB_TOL, r_it.size), r0


def _raw(fr, r, st, ph, W, H, shard, planes, layout, precision):
    p = st.to_params(fr.FractalType.Phoenix, precision)
    cph = ph.to_c()
    o = fr._capi.fr_output(planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), fr._capi.FR_MEM_DEVICE, layout)
    sh = shard.to_c()
    return fr.lib().fr_render_phoenix(r._ctx, C.byref(p), C.byref(cph), W, H, C.byref(sh), C.byref(o))


@pytest.mark.parametrize("f64", [False, True])
def test_shards_reassemble_the_frame(fr, renderer, f64):
    import torch
    W, H = 203, 117
    st = fr.FractalState(max_iterations=200, center_x=-0.3, zoom=2.5)
    ph = fr.PHOENIX_PRESETS["Swirl"]
    prec = fr.Precision.F64 if f64 else fr.Precision.F32
    whole = _render(fr, renderer, st, ph, W, H, prec)
    dev = torch.device("cuda:0")
    tdt = torch.float64 if f64 else torch.float32
    for nparts in (1, 2, 3, 8):
        for R in (1, 8, 13):
            frame = [torch.full((H, W, 4), -1.0, device=dev), torch.full((H, W), -1.0, dtype=tdt, device=dev),
                     torch.full((H, W), -1, dtype=torch.int32, device=dev)]
            packed = [np.zeros((H, W, 4), np.float32), np.zeros((H, W), whole[1].dtype), np.zeros((H, W), np.int32)]
            for part in range(nparts):
                shard = fr.Shard(part, nparts, R)
                rows = shard.rows(H)
                if rows == 0:
                    continue
                g = shard.global_rows(H)
                h = _render(fr, renderer, st, ph, W, H, prec, shard=shard)
                d = [torch.empty((rows, W, 4), device=dev), torch.empty((rows, W), dtype=tdt, device=dev),
                     torch.empty((rows, W), dtype=torch.int32, device=dev)]
                renderer.render_phoenix(st, W, H, ph, precision=prec, rgba=d[0], nu=d[1], iter=d[2], shard=shard)
                for k in range(3):
                    assert np.array_equal(d[k].cpu().numpy(), h[k]), (nparts, R, part, k)   # host planes == device planes
                    packed[k][g] = h[k]
                assert _raw(fr, renderer, st, ph, W, H, shard, frame, fr._capi.FR_LAYOUT_FRAME, prec) == 0
            for k in range(3):
                assert packed[k].tobytes() == whole[k].tobytes(), (nparts, R, k)
                assert frame[k].cpu().numpy().tobytes() == whole[k].tobytes(), (nparts, R, k)
    # a part that owns no rows: the synchronous entries have nothing to do; the asynchronous ones refuse host planes
    # before they look at the shard, for Phoenix as for the escape-time kernels
    E, L = fr._capi, fr.lib()
    none = fr.Shard(2, 3, 64)
    assert none.rows(H) == 0
    empty = none.to_c()
    host = E.fr_output(packed[0].ctypes.data, packed[1].ctypes.data, packed[2].ctypes.data, E.FR_MEM_HOST, E.FR_LAYOUT_PACKED)
    p, cph = st.to_params(fr.FractalType.Phoenix, prec), ph.to_c()
    q = st.to_params(fr.FractalType.Mandelbrot, prec)
    assert L.fr_render_phoenix(renderer._ctx, C.byref(p), C.byref(cph), W, H, C.byref(empty), C.byref(host)) == E.FR_OK
    assert L.fr_render_shard(renderer._ctx, C.byref(q), W, H, C.byref(empty), C.byref(host)) == E.FR_OK
    assert L.fr_render_phoenix_async(renderer._ctx, C.byref(p), C.byref(cph), W, H, C.byref(empty), C.byref(host),
                                     None) == E.FR_ERR_INVALID_ARG
    assert L.fr_render_shard_async(renderer._ctx, C.byref(q), W, H, C.byref(empty), C.byref(host), None) == E.FR_ERR_INVALID_ARG


def test_async_back_to_back_on_a_torch_stream(fr, renderer):
    import torch
    W, H = 640, 480
    dev = torch.device("cuda:0")
    sts = [(fr.FractalState(max_iterations=300), fr.PhoenixParams()),
           (fr.FractalState(max_iterations=200, zoom=1.2, stripe_density=4.0), fr.PHOENIX_PRESETS["Chaos"])]
    want = [_render(fr, renderer, st, ph, W, H, fr.Precision.F32) for st, ph in sts]
    s = torch.cuda.Stream()
    outs = [[torch.empty((H, W, 4), device=dev), torch.empty((H, W), device=dev),
             torch.empty((H, W), dtype=torch.int32, device=dev)] for _ in sts]
    with torch.cuda.stream(s):
        for (st, ph), o in zip(sts, outs):
            renderer.render_phoenix(st, W, H, ph, precision=fr.Precision.F32, rgba=o[0], nu=o[1], iter=o[2], sync=False,
                                    stream=s.cuda_stream)
    s.synchronize()
    renderer.check()
    assert renderer.last_kernel_ms() > 0.0 and renderer.last_grid() > 0 and renderer.last_stages() == 1
    for w, o in zip(want, outs):
        for k in range(3):
            assert np.array_equal(o[k].cpu().numpy(), w[k])


@pytest.mark.parametrize("jc", [(float(np.float32(-0.7)), float(np.float32(0.27015))), (0.6, 0.55)])
def test_julia_mode_frame_is_constant(fr, renderer, jc):
    W, H = 96, 64
    st = fr.FractalState(max_iterations=128, julia_c_real=jc[0], julia_c_imag=jc[1])
    ph = fr.PhoenixParams(use_julia_set=True)
    for post in (False, True):
        rgba, nu, it = _render(fr, renderer, st, ph, W, H, fr.Precision.F32, post=post)
        assert np.all(rgba == rgba[0, 0]) and np.all(nu == nu[0, 0]) and np.all(it == it[0, 0])
        r_it, r_sm, r_rgb = phoenix_ref.render(4, 4, max_iterations=128, julia_c_real=jc[0], julia_c_imag=jc[1],
                                               use_julia_set=True, post=post)
        assert it[0, 0] == r_it[0, 0] and _ulp_ok(nu[0, 0], r_sm[0, 0])
        assert np.abs(rgba[0, 0, :3] - r_rgb[0, 0]).max() <= RGB_TOL


def test_no_interference_with_other_kernels(fr):
    import torch
    W, H = 512, 384
    dev = torch.device("cuda:0")

    def mandel(r):
        o = [torch.empty((H, W, 4), device=dev), torch.empty((H, W), dtype=torch.float64, device=dev),
             torch.empty((H, W), dtype=torch.int32, device=dev)]
        r.render(fr.FractalState(max_iterations=1024), W, H, rgba=o[0], nu=o[1], iter=o[2])
        return [x.cpu().numpy() for x in o]

    with fr.Renderer(0) as fresh:
        want = mandel(fresh)
    with fr.Renderer(0) as r:
        a = mandel(r)
        _render(fr, r, fr.FractalState(max_iterations=512), fr.PhoenixParams(), W, H, fr.Precision.F64)
        b = mandel(r)
    for k in range(3):
        assert a[k].tobytes() == want[k].tobytes() and b[k].tobytes() == want[k].tobytes()


def test_long_orbits_complete(fr, renderer):
    W, H, max_iter = 32, 24, 1 << 20
    st = fr.FractalState(max_iterations=max_iter, center_x=0.0, center_y=0.0, zoom=0.6)
    rgba, nu, it = _render(fr, renderer, st, fr.PhoenixParams(), W, H, fr.Precision.F32)
    short = phoenix_ref.render(W, H, max_iterations=128, center_x=0.0, center_y=0.0, zoom=0.6)[0]
    assert np.array_equal(it[short < 128], short[short < 128])      # escapes before 128 are the same escapes
    assert (it == max_iter).mean() > 0.5 and np.all(nu[it == max_iter] == max_iter)
    assert not np.isnan(rgba).any()
