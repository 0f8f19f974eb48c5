"""phoenix_orbit (fr_phoenix.hip.h) at its block boundaries and re-entries, against the numpy restatement: unchecked blocks
of 16 updates followed by a tested tail, the replay of a block, lanes parked at z = z_prev = C = 0, lanes without a sample,
and the fp64 kernel's narrowing into the float colour stage.  The cases and what each of them can see are data and CPU
predicates in phoenix_cases.py, asserted by test_phoenix_host.py::test_orbit_cases_can_fail; the bars are those of
test_phoenix_gpu.py, imported: iter bit for bit, nu within NU_TOL_F64 (fp64) or _ulp_ok (fp32), colour within RGB_TOL on all
but _few pixels, alpha exactly 1.  Every render goes into planes pre-filled with a sentinel.

Three deliberately wrong variants of phoenix_orbit, so far only in a numpy emulation of its control flow (a wave taken as an
aligned 8x8 tile; not yet as builds on a GPU): a tail that stops one update early gets exactly the samples that escape in
the last update wrong (26 of the 28 boundary cases with a tail; Classic has no such sample at max_iter 47); a block that
tests only its last |z|^2 loses the lanes that reached NaN unless a neighbour's escape replays the block (every fp32 case
with a full block, 27 to 35 of the re-entering samples); a rollback that keeps z_prev fails every case with a full block.
"""
import numpy as np
import pytest

import phoenix_cases as pc
from test_phoenix_gpu import NU_TOL_F64, RGB_TOL, _few, _ulp_ok

pytestmark = pytest.mark.gpu

SENTINEL = -7


def _ids(cases):
    return dict(argvalues=list(cases.values()), ids=list(cases))


def gpu_render(fr, renderer, case, W=None, H=None):
    """the case on the GPU (optionally at another frame size), in device planes pre-filled with SENTINEL"""
    import torch
    kw = case[2]
    W, H = W or case[0], H or case[1]
    f64 = kw["f64"]
    st = fr.FractalState(max_iterations=kw["max_iterations"], antialiasing_samples=kw.get("aa", 1),
                         **{k: kw[k] for k in ("center_x", "center_y", "zoom", "julia_c_real", "julia_c_imag", "stripe_density",
                                               "color_brightness", "color_saturation", "color_contrast") if k in kw})
    ph = fr.PhoenixParams(kw.get("phoenix_p", 0.0), kw.get("phoenix_r", -0.5), bool(kw.get("use_julia_set", False)))
    dev = torch.device("cuda:0")
    rgba = torch.full((H, W, 4), float(SENTINEL), dtype=torch.float32, device=dev)
    nu = torch.full((H, W), float(SENTINEL), dtype=torch.float64 if f64 else torch.float32, device=dev)
    it = torch.full((H, W), SENTINEL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()            # the fills run on torch's stream, the render on the context's own
    renderer.render_phoenix(st, W, H, ph, precision=fr.Precision.F64 if f64 else fr.Precision.F32,
                            post_chain=bool(kw.get("post", False)), rgba=rgba, nu=nu, iter=it)
    return rgba.cpu().numpy(), nu.cpu().numpy(), it.cpu().numpy()


def check_orbit(case, planes, what=None):
    """iter and nu of a render against the case's reference"""
    _, nu, it = planes
    r_it, r_sm, _ = pc.reference(case)
    what = what or case[2]
    wrong = it != r_it
    assert not wrong.any(), (what, int(wrong.sum()), "first at (y, x)", tuple(map(int, np.argwhere(wrong)[0])),
                             "gpu", int(it[wrong][0]), "ref", int(r_it[wrong][0]))
    if case[2]["f64"]:
        assert np.abs(nu - r_sm).max() <= NU_TOL_F64, (what, float(np.abs(nu - r_sm).max()))
    else:
        assert np.all(_ulp_ok(nu, r_sm)), (what, float(np.abs(nu.astype(np.float64) - r_sm).max()))


def bad_pixels(case, planes, what=None):
    """alpha exactly 1, no NaN; returns the mask of the pixels whose colour is further than RGB_TOL from the reference's"""
    rgba = planes[0]
    r_rgb = pc.reference(case)[2]
    assert not np.isnan(rgba).any() and np.all(rgba[..., 3] == 1.0), what or case[2]
    return np.abs(rgba[..., :3] - r_rgb).max(axis=2) > RGB_TOL


def check(case, planes, what=None):
    check_orbit(case, planes, what)
    bad = bad_pixels(case, planes, what)
    assert _few(bad, bad.size), (what or case[2], int(bad.sum()))


@pytest.mark.parametrize("case", **_ids(pc.BOUNDARY))
def test_block_boundaries(fr, renderer, case):
    """max_iter just below, at and just above every multiple of 16 up to 63: no block at all, full blocks and no tail, full
    blocks and a tail of one or of fifteen -- with escapes in every block and in the tail (test_orbit_cases_can_fail)."""
    check(case, gpu_render(fr, renderer, case))


@pytest.mark.parametrize("case", **_ids(pc.REENTRY))
def test_reentering_orbits_escape_where_the_shader_breaks(fr, renderer, case):
    """Orbits that leave the disc and, continued, are back inside it before their block of 16 ends: the shader broke at the
    first escape, so the kernel may neither miss it (testing the block's last |z|^2 only) nor report a later one."""
    planes = gpu_render(fr, renderer, case)
    back = pc.reentering(case)
    it, r_it = planes[2], pc.reference(case)[0]
    wrong = (it != r_it) & back
    assert not wrong.any(), "%d of the %d re-entering samples escape elsewhere than in the shader (first: gpu %d, ref %d)" % (
        int(wrong.sum()), int(back.sum()), int(it[wrong][0]), int(r_it[wrong][0]))
    check(case, planes)


@pytest.mark.parametrize("case", **_ids(pc.RAGGED))
def test_ragged_frames_park_lanes_without_samples(fr, renderer, case):
    """Frames that fill no 8x8 sub-tile: lanes outside the frame run with C = 0 and live = false next to live lanes; a parked
    lane must never make its wave leave early and never hold it."""
    planes = gpu_render(fr, renderer, case)
    check_orbit(case, planes)
    bad = bad_pixels(case, planes)
    if bad.size == 1:               # _few's floor of 2 would pass anything here: the CPU decides whether the colour may move
        assert pc.near_wrap(case) > 0 or not bad.any(), case[2]
    else:
        assert _few(bad, bad.size), (case[2], int(bad.sum()))


@pytest.mark.parametrize("aa", [1, 2, 3])
@pytest.mark.parametrize("max_iter", [33, 80])
def test_fp64_colour_stage_matches_the_restatement(fr, renderer, max_iter, aa):
    """t = smooth / max_iter divided in double and narrowed, the smooth count and lastZ narrowed, then the float colour stage:
    under supersampling (iter and nu are those of sample (0,0)), with the post chain off, on and at its floors, with the
    stripes off (0, 0.005: below the 0.01 switch) and on (10, 17.5: amp 0.5 and 0.875)."""
    seen = 0
    for name, case in pc.COLOUR_F64.items():
        kw = case[2]
        if (kw["max_iterations"], kw["aa"]) == (max_iter, aa):
            check(case, gpu_render(fr, renderer, case), name)
            seen += 1
    assert seen == len(pc.POSTS) * len(pc.DENSITIES)


@pytest.mark.parametrize("max_iter", [17, 128])
@pytest.mark.parametrize("k", [0, 1])
def test_fp64_julia_mode(fr, renderer, k, max_iter):
    """test_julia_mode_frame_is_constant in fp64: every lane of every wave runs the same orbit (jc 0 never escapes, jc 1
    escapes in the first block), so the frame is one value in every plane, and that value is the restatement's."""
    W, H = 96, 64
    seen = 0
    for name, case in pc.JULIA_F64.items():
        kw = case[2]
        if (kw["julia_c_real"], kw["julia_c_imag"]) == pc.JULIA_C[k] and kw["max_iterations"] == max_iter:
            rgba, nu, it = gpu_render(fr, renderer, case, W, H)
            assert np.all(rgba == rgba[0, 0]) and np.all(nu == nu[0, 0]) and np.all(it == it[0, 0]), name
            r_it, r_sm, r_rgb = pc.reference(case)
            assert it[0, 0] == r_it[0, 0] and abs(nu[0, 0] - r_sm[0, 0]) <= NU_TOL_F64, name
            assert rgba[0, 0, 3] == 1.0 and np.abs(rgba[0, 0, :3] - r_rgb[0, 0]).max() <= RGB_TOL, name
            seen += 1
    assert seen == 2


@pytest.mark.parametrize("case", **_ids(pc.INTERIOR))
def test_interior_last_z_feeds_the_stripes(fr, renderer, case):
    """A sample that never escapes takes lastZ from the live registers after the tail (max_iter 33: one update after two
    blocks, 47: fifteen), and the stripes read its angle.  The interior pixels are counted on their own, so that an error
    in them alone is not diluted into the allowance of the whole frame."""
    planes = gpu_render(fr, renderer, case)
    check_orbit(case, planes)
    bad = bad_pixels(case, planes)
    interior = pc.reference(case)[0] == case[2]["max_iterations"]
    assert _few(bad[interior], int(interior.sum())), (case[2], int(bad[interior].sum()), int(interior.sum()))
    assert _few(bad, bad.size), (case[2], int(bad.sum()))
