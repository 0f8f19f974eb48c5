"""Mandelbulb on the GPU (fr_render_mandelbulb): against the executed shader, the numpy restatement at realistic sizes,
shards, host and device planes, the asynchronous form, the NaN policy, and its coexistence with the other kernels.

Tolerances.  The kernel evaluates the shader's operations in the shader's order with OCML's acosf, atan2f, powf, sinf,
cosf, expf and logf; the fixture and the restatement use numpy's float32 functions.  They differ by an ulp here and
there, and the ray march amplifies that: a ray grazing the surface can flip hit / miss, a step count can move by one,
and the palette's hash (fract(sin(.) * 43758.5)) turns an ulp of its argument into a visible colour change.  On the host,
restatement and interpreter agree bitwise (tests/test_mandelbulb_host.py).  Evidence for the bounds: in the first
MI355X run of this suite every pixel of all 18 fixture cases was within RGB_TOL of the executed shader (0 pixels over,
printed by test_fixture_cases), and every bound below held.  The bounds keep a margin for other hosts' numpy and
later compilers:
  - hit / miss and step index may differ on MAX_FLIP of the pixels (and at least 2 per case);
  - post-chained RGB within RGB_TOL on all but MAX_FLIP of the pixels.
"""
import ctypes as C

import numpy as np
import pytest

import mandelbulb_ref
from test_mandelbulb_host import mbx, params_of   # noqa: F401  (mbx: the fixture)

pytestmark = pytest.mark.gpu

MAX_FLIP = 0.02         # share of pixels whose hit / miss, step or colour may differ from the CPU's
RGB_TOL = 2e-3          # post-chained RGB elsewhere


def _render(fr, r, st, mb, W, H, post=False, shard=None):
    rows = shard.rows(H) if shard else H
    rgba = np.empty((rows, W, 4), np.float32)
    nu = np.empty((rows, W), np.float32)
    it = np.empty((rows, W), np.int32)
    r.render_mandelbulb(st, W, H, mb, post_chain=post, rgba=rgba, nu=nu, iter=it, shard=shard)
    return rgba, nu, it


def _few(bad, n):
    return int(bad.sum()) <= max(2, int(MAX_FLIP * n))


def _post_policy(ref_rgb):
    """the fixture's texel under the NaN policy: a NaN colour is black after the post chain"""
    return np.where(np.isnan(ref_rgb).any(-1, keepdims=True), np.float32(0.0), ref_rgb)


def test_fixture_cases(fr, renderer, mbx):   # noqa: F811
    stats = {}
    for name, (W, H, p, pc, rgba_ref, lin_ref, it_ref, t_ref) in mbx.items():
        st, mb = params_of(fr, p)
        rgba, nu, it = _render(fr, renderer, st, mb, W, H, post=True)
        assert not np.isnan(rgba).any(), name                       # the post-chained plane is finite
        assert np.all(rgba[..., 3] == 1.0)
        ref = _post_policy(rgba_ref[..., :3])
        bad = np.abs(rgba[..., :3] - ref).max(-1) > RGB_TOL
        n = W * H
        stats[name] = int(bad.sum())
        assert _few(bad, n), (name, int(bad.sum()))
        if it_ref is not None:
            assert _few((it >= 0) != (it_ref >= 0), n), name
            assert _few(it != it_ref, n), name
            same = it == it_ref
            assert np.allclose(nu[same], t_ref[same], rtol=1e-4, atol=1e-5) or _few(~np.isclose(nu, t_ref, 1e-4, 1e-5), n)
            lin, _, _ = _render(fr, renderer, st, mb, W, H, post=False)
            # the linear plane carries the shader's NaN
            assert _few(np.isnan(lin[..., :3]).any(-1) != np.isnan(lin_ref).any(-1), n), name
    print("pixels over RGB_TOL per case:", stats)


@pytest.mark.parametrize("W,H", [(1700, 900), (1920, 1080)])
def test_realistic_sizes_against_the_restatement(fr, renderer, W, H):
    st = fr.FractalState(max_iterations=64)
    mb = fr.MandelbulbParams(time=1.25)
    rgba, nu, it = _render(fr, renderer, st, mb, W, H, post=True)
    assert not np.isnan(rgba).any()
    for r0 in (0, H // 2 - 4, H - 8):
        band = (r0, r0 + 8)
        r_it, r_t, r_lin = mandelbulb_ref.render(W, H, rows=band, max_iterations=64, time=1.25)
        n = r_it.size
        assert _few((it[r0:r0 + 8] >= 0) != (r_it >= 0), n), r0
        ref = mandelbulb_ref.post_chain(r_lin)
        bad = np.abs(rgba[r0:r0 + 8, :, :3] - ref).max(-1) > RGB_TOL
        assert _few(bad, n), (r0, int(bad.sum()))


def test_split_and_in_loop_shading_are_bitwise_equal(fr, renderer):
    W, H = 320, 200
    st, mb = fr.FractalState(max_iterations=48, antialiasing_samples=2), fr.MandelbulbParams(time=0.6)
    a = _render(fr, renderer, st, mb, W, H)
    renderer.set_option("mandelbulb_split", 1)
    try:
        b = _render(fr, renderer, st, mb, W, H)
    finally:
        renderer.set_option("mandelbulb_split", 0)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_shards_reassemble_the_frame(fr, renderer):
    import torch
    W, H = 200, 150
    st, mb = fr.FractalState(max_iterations=32), fr.MandelbulbParams(mandelbulb_power=6.0)
    whole = _render(fr, renderer, st, mb, W, H, post=True)
    for nparts, rps in ((3, 0), (4, 16)):
        rgba = np.empty((H, W, 4), np.float32)
        nu = np.empty((H, W), np.float32)
        it = np.empty((H, W), np.int32)
        for part in range(nparts):
            sh = fr.Shard(part, nparts, rps)
            a, b, c = _render(fr, renderer, st, mb, W, H, post=True, shard=sh)
            rows = sh.global_rows(H)
            rgba[rows], nu[rows], it[rows] = a, b, c
        assert rgba.tobytes() == whole[0].tobytes() and nu.tobytes() == whole[1].tobytes()
        assert it.tobytes() == whole[2].tobytes()
    # FR_LAYOUT_FRAME: every part writes its own rows of one device frame
    dev = torch.device("cuda:0")
    frame = [torch.full((H, W, 4), -7.0, dtype=torch.float32, device=dev), torch.zeros((H, W), dtype=torch.float32, device=dev),
             torch.zeros((H, W), dtype=torch.int32, device=dev)]
    p = st.to_params(fr.FractalType.Mandelbulb, fr.Precision.F32, True)
    cmb = mb.to_c()
    o = fr._capi.fr_output(frame[0].data_ptr(), frame[1].data_ptr(), frame[2].data_ptr(), fr._capi.FR_MEM_DEVICE,
                           fr._capi.FR_LAYOUT_FRAME)
    for part in range(3):
        sh = fr.Shard(part, 3, 8).to_c()
        assert fr.lib().fr_render_mandelbulb(renderer._ctx, C.byref(p), C.byref(cmb), W, H, C.byref(sh), C.byref(o)) == 0
    for k in range(3):
        assert frame[k].cpu().numpy().tobytes() == whole[k].tobytes(), k


def test_host_planes_equal_device_planes_and_async(fr, renderer):
    import torch
    W, H = 160, 120
    st, mb = fr.FractalState(max_iterations=40), fr.MandelbulbParams(time=2.0)
    host = _render(fr, renderer, st, mb, W, H)
    dev = torch.device("cuda:0")
    rgba = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    nu = torch.empty((H, W), dtype=torch.float32, device=dev)
    it = torch.empty((H, W), dtype=torch.int32, device=dev)
    renderer.render_mandelbulb(st, W, H, mb, rgba=rgba, nu=nu, iter=it)
    assert rgba.cpu().numpy().tobytes() == host[0].tobytes()
    assert nu.cpu().numpy().tobytes() == host[1].tobytes() and it.cpu().numpy().tobytes() == host[2].tobytes()
    s = torch.cuda.Stream(device=dev)
    for t in (rgba, nu, it):
        t.zero_()
    torch.cuda.synchronize()
    renderer.render_mandelbulb(st, W, H, mb, rgba=rgba, nu=nu, iter=it, stream=s.cuda_stream, sync=False)
    s.synchronize()
    assert rgba.cpu().numpy().tobytes() == host[0].tobytes() and it.cpu().numpy().tobytes() == host[2].tobytes()


def test_nan_policy(fr, renderer):
    """the default view: many hits inside the unit sphere.  Linear plane: NaN there; post-chained plane: black, finite."""
    W, H = 96, 72
    st, mb = fr.FractalState(max_iterations=64), fr.MandelbulbParams()
    lin, _, it = _render(fr, renderer, st, mb, W, H)
    post, _, _ = _render(fr, renderer, st, mb, W, H, post=True)
    nan = np.isnan(lin[..., :3]).any(-1)
    assert nan.any() and np.all(it[nan] >= 0)
    assert not np.isnan(post).any()
    assert np.all(post[nan][:, :3] == 0.0)


def test_other_kernels_unchanged_by_a_mandelbulb_render(fr, renderer):
    W, H = 256, 192

    def others():
        st = fr.FractalState(max_iterations=200)
        a = np.empty((H, W, 4), np.float32)
        renderer.render(st, W, H, precision=fr.Precision.F32, rgba=a)
        b = np.empty((H, W, 4), np.float32)
        renderer.render_phoenix(st, W, H, rgba=b)
        return a.tobytes(), b.tobytes()

    before = others()
    _render(fr, renderer, fr.FractalState(max_iterations=32), fr.MandelbulbParams(), W, H)
    assert others() == before
