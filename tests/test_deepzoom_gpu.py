"""deep_zoom_kernel (fr_kernels.hip.h) at its loop tails, phase joins and palettes, against the CPU oracle: the perturbed
phase over orbit[0 .. n_ref) and the plain phase over [n_ref, max_iter), each a loop over groups of four updates behind a
wave-wide ballot followed by a tested tail; the join from orbit[ref_iter - 1] + dz, or from c without an orbit; lanes without
a sample; the bailout clamp; the four palettes; the orbit buffer from one render to the next; every entry point that reaches
the kernel.  The cases and what each of them can see are data and CPU predicates in deepzoom_cases.py, asserted by
test_deepzoom_cases_host.py; the bars are check_against's of test_gpu_parity.py, unchanged: iter bit for bit, nu within
4 ulp + 4e-6, colour within RGB_TOL plus the fp32 term, at most max(2, 0.1 %) palette-wrap exceptions per frame.  Every
render goes into planes pre-filled with a sentinel (gpu_render).

Nine one-line mutants of deep_zoom_kernel were built and run against this file and against the Deep_Zoom tests that existed
before it (the four cases of cases.py in test_case_matches_oracle_and_golden, the SPIR-V fixtures,
test_deep_zoom_larger_frame_and_planes); the commit that added this file lists which tests saw which mutant.
"""
import numpy as np
import pytest

import deepzoom_cases as dc
from test_gpu_parity import RGB_TOL, check_against, gpu_render, to_state

pytestmark = pytest.mark.gpu


def _ids(cases):
    return dict(argvalues=list(cases), ids=list(cases))


def _check(fr, renderer, case, what, shard=None):
    """one case on the GPU against its reference; returns the GPU planes"""
    p, W, H = case
    ref = dc.reference(case)
    sh = fr.Shard(*shard) if shard else None
    planes = gpu_render(fr, renderer, p, W, H, shard=sh)
    rows = sh.global_rows(H) if sh else slice(None)
    try:
        check_against(p, ref.iter[rows], ref.nu[rows], ref.rgba[rows], *planes)
    except AssertionError as e:
        raise AssertionError("%s %r %dx%d shard %r: %s" % (what, p, W, H, shard, e))
    return planes


@pytest.mark.parametrize("cid", **_ids(dc.REMAINDER))
def test_remainders_of_both_phases(fr, renderer, cid):
    """Perturbed renders whose orbit ends at L, L % 4 = 0..3, with max_iter = L + 0..7: every remainder of the perturbed
    phase's tail against every length of the plain phase (no group of four, one group, each tail), with escapes at every
    update of both tails and in the last update of all (test_remainder_cases_put_escapes_into_both_tails)."""
    _check(fr, renderer, dc.REMAINDER[cid], cid)


@pytest.mark.parametrize("cid", **_ids(dc.INTERIOR_CENTRE))
def test_orbit_as_long_as_max_iter(fr, renderer, cid):
    """The centre never leaves: n_ref = max_iter = 1..9, the plain phase is empty and starts (and ends) behind the join."""
    _check(fr, renderer, dc.INTERIOR_CENTRE[cid], cid)


@pytest.mark.parametrize("cid", **_ids(dc.NO_ORBIT))
def test_plain_phase_alone(fr, renderer, cid):
    """use_perturbation = 0: no orbit is read, the plain phase starts from z = c at k = 0 and holds escapes at every update."""
    _check(fr, renderer, dc.NO_ORBIT[cid], cid)


@pytest.mark.parametrize("cid", **_ids(dc.RAGGED))
def test_ragged_frames_start_lanes_dead(fr, renderer, cid):
    """Frames that fill no 8x8 sub-tile: a lane without a sample starts dead next to live ones; it must neither hold its wave
    nor let it leave early, and stores nothing.  One pixel: check_against's floor of two exceptions would let any colour
    pass, so a 1x1 frame's colour is held to the bar without the exception (its reference is nowhere near the wrap:
    test_ragged_cases_leave_lanes_without_a_sample)."""
    case = dc.RAGGED[cid]
    p, W, H = case
    rgba, nu, it = _check(fr, renderer, case, cid)
    if W * H == 1:
        ref = dc.reference(case)
        tol = RGB_TOL + 5.0 * abs(p.color_scale) / p.max_iterations * 8e-6
        assert np.abs(rgba - ref.rgba).max() <= tol, cid


@pytest.mark.parametrize("cid", **_ids(dc.WAVE_EXIT))
def test_waves_that_leave_early_next_to_waves_that_stay(fr, renderer, cid):
    """Sub-tiles fully escaped before the last group of four (the break, no tail, the plain phase's break at once), sub-tiles
    with an escape in the first group and a sample that runs to the end, and sub-tiles that are wholly interior."""
    _check(fr, renderer, dc.WAVE_EXIT[cid], cid)


@pytest.mark.parametrize("view", list(dc.COLOUR_VIEWS))
@pytest.mark.parametrize("palette", dc.PALETTES)
def test_palettes_scales_and_bailouts(fr, renderer, view, palette):
    """palette_mode -1..4 (0, 1, 2 and the grey fall-back, each with its own fract factor) x colour scale 1, -2.5, 6 and 0
    x bailout 0.5 (clamped to 2), 2, 4, 1e4 and 3e19 (bailout^2 = inf: every sample interior while its z runs to inf and
    NaN), on a perturbed and an unperturbed view.  No reference holds more samples next to the palette's wrap than
    check_against's exception lets pass (test_colour_cases_stay_clear_of_the_palette_wrap)."""
    seen = 0
    for cid, key in dc.COLOUR_KEYS.items():
        if key[:2] == (view, palette):
            rgba, nu, it = _check(fr, renderer, dc.COLOUR[cid], cid)
            assert np.isfinite(rgba).all() and np.isfinite(nu).all(), cid
            seen += 1
    assert seen == len(dc.SCALE_OFFSET) * len(dc.BAILOUTS)


def test_seeded_sweep(fr, renderer):
    """test_randomised_views_match_the_oracle for Deep_Zoom alone: 32 trials over views around the Mandelbrot boundary,
    max_iter around the groups of four, perturbation on and off, palettes -1..4, bailouts from under the clamp to 1000,
    ragged sizes, a row-strip shard every third trial."""
    for cid, (p, W, H, shard) in dc.SWEEP.items():
        _check(fr, renderer, (p, W, H), cid, shard=shard)


# ---- beyond single frames -----------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_orbit_buffer_across_renders_of_one_context(fr):
    """A long orbit, short ones behind it, a render without an orbit, a longer one that grows the buffers, the first short
    one again -- on ONE context: every frame matches the oracle and is byte-identical to the same frame rendered first on a
    fresh context.  A short orbit must never see a longer predecessor's points."""
    got = []
    with fr.Renderer(0) as one:
        for k, case in enumerate(dc.ORBIT_SEQUENCE):
            got.append(_check(fr, one, case, "render %d of the sequence" % k))
    for k, case in enumerate(dc.ORBIT_SEQUENCE):
        with fr.Renderer(0) as fresh:
            want = gpu_render(fr, fresh, *case)
        assert _same(got[k], want), "render %d of the sequence differs from a fresh context's" % k


@pytest.mark.parametrize("cid", **_ids(dc.ENTRY_POINT_CASES))
def test_every_entry_point_gives_the_same_planes(fr, renderer, cid):
    """Host planes, single planes, an asynchronous render on a torch stream with a dependent op behind it, a reserved
    context, row-strip shards, the whole-frame layout through a node of two lanes, and queue options that must never change
    a pixel: byte-identical to the plain device render, which matches the oracle."""
    import torch
    case = dc.ENTRY_POINT_CASES[cid]
    p, W, H = case
    base = _check(fr, renderer, case, cid)
    st = to_state(fr, p)
    kw = dict(fractal_type=fr.FractalType.Deep_Zoom, precision=fr.Precision.F32)

    def planes(rows=H, fill=-7):
        out = (torch.full((rows, W, 4), float(fill), dtype=torch.float32, device="cuda:0"),
               torch.full((rows, W), float(fill), dtype=torch.float32, device="cuda:0"),
               torch.full((rows, W), fill, dtype=torch.int32, device="cuda:0"))
        torch.cuda.synchronize()
        return out

    def host(ts):
        return tuple(t.cpu().numpy() for t in ts)

    # FR_MEM_HOST
    assert _same(base, gpu_render(fr, renderer, p, W, H, host=True)), "host planes"
    # one plane at a time
    for k, name in enumerate(("rgba", "nu", "iter")):
        out = planes()
        renderer.render(st, W, H, **kw, **{name: out[k]})
        assert _same(base[k:k + 1], host(out[k:k + 1])), name + " only"
    # sync=False on a torch stream, a dependent op queued behind the render
    s = torch.cuda.Stream()
    out = planes()
    with torch.cuda.stream(s):
        renderer.render(st, W, H, **kw, rgba=out[0], nu=out[1], iter=out[2], sync=False, stream=s.cuda_stream)
        doubled = out[1] * 2
        shifted = out[2] + 1
    s.synchronize()
    assert _same(base, host(out)), "async"
    assert np.array_equal(doubled.cpu().numpy(), base[1] * np.float32(2)) and np.array_equal(shifted.cpu().numpy(), base[2] + 1)
    # a context that reserved first
    with fr.Renderer(0) as r:
        r.reserve(st, W, H, **kw)
        out = planes()
        r.render(st, W, H, **kw, rgba=out[0], nu=out[1], iter=out[2])
        assert _same(base, host(out)), "after reserve"
    # row strips: the packed rows are the whole frame's
    for nparts, R in ((2, 8), (3, 16), (5, 1)):
        for part in range(nparts):
            sh = fr.Shard(part, nparts, R)
            rows = sh.global_rows(H)
            if len(rows):
                got = gpu_render(fr, renderer, p, W, H, shard=sh)
                assert _same(tuple(b[rows] for b in base), got), ("strips", nparts, R, part)
    # the whole-frame layout: two lanes of this card store their strips in place
    with fr.Node([0, 0]) as node:
        out = planes()
        node.render(st, W, H, **kw, rgba=out[0], nu=out[1], iter=out[2])
        assert _same(base, host(out)), "node"
    # options that must never change a pixel
    try:
        renderer.set_option("shards", 64)
        assert _same(base, gpu_render(fr, renderer, p, W, H)), "shards 64"
        renderer.set_option("shards", 0)
        for shape in (3, 4, 6):
            renderer.set_tuning(shape=shape)
            assert _same(base, gpu_render(fr, renderer, p, W, H)), ("shape", shape)
    finally:
        renderer.set_option("shards", 0)
        renderer.set_tuning()
