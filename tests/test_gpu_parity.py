"""Parity of the HIP path (through the C ABI) against the CPU oracle and the golden fixtures.

Bars:
  * escape index `iter`: bit-exact (integer) in fp64 AND fp32 -- both sides perform the same IEEE
    operations in the same order, no contraction;
  * smooth iteration count nu, fp64: |dnu| <= 1e-9 asserted (the north-star tolerance is 1e-6); the
    only difference is the log() implementation (OCML vs glibc), a few ulp;
  * nu, fp32: |dnu| <= 4 ulp32(nu) + 4e-6 (same reason, in float);
  * colour: |d| <= 2e-5 per channel (powf/expf implementations; fp32 adds the nu tolerance times the slope
    5 * color_scale / max_iter with which it reaches the palette -- nothing unless max_iter is a handful), except
    pixels whose palette argument sits within 1e-4 of the fract() wrap, where a 1-ulp nu difference legitimately
    flips the colour (fp32, one sample per pixel only; the fp64 planes never hit it).  With the post chain the bar
    is 1e-4, and pixels next to black, where the final pow(c, 1/2.2) has unbounded slope, are compared before the
    gamma (1e-6).
"""
import ctypes as C
import os

import numpy as np
import pytest

from cases import CASES, MANDEL_PALETTES, JULIA_PALETTES, needs_effects
from spv_cases import SPV_CASES

pytestmark = pytest.mark.gpu

NU_TOL_F64 = 1e-9
RGB_TOL = 2e-5


def to_state(fr, p):
    return fr.FractalState(center_x=p.center_x, center_y=p.center_y, zoom=p.zoom, max_iterations=p.max_iterations,
                           julia_c_real=p.julia_c_real, julia_c_imag=p.julia_c_imag, bailout=p.bailout,
                           antialiasing_samples=p.aa, palette_mode=p.palette_mode, color_offset=p.color_offset,
                           color_scale=p.color_scale, interior_style=p.interior_style,
                           orbit_trap_enabled=bool(p.orbit_trap_enabled), orbit_trap_radius=p.orbit_trap_radius,
                           stripe_enabled=bool(p.stripe_enabled), stripe_density=p.stripe_density,
                           color_brightness=p.brightness, color_saturation=p.saturation, color_contrast=p.contrast,
                           use_perturbation=bool(p.use_perturbation))


def gpu_render(fr, renderer, p, W, H, shard=None, host=False):
    import torch
    prec = fr.Precision.F64 if p.precision == 1 else fr.Precision.F32
    rows = shard.rows(H) if shard else H
    if host:
        rgba = np.full((rows, W, 4), -7.0, np.float32)
        nu = np.full((rows, W), -7.0, np.float64 if p.precision == 1 else np.float32)
        it = np.full((rows, W), -7, np.int32)
    else:
        dev = torch.device("cuda:0")
        rgba = torch.full((rows, W, 4), -7.0, dtype=torch.float32, device=dev)
        nu = torch.full((rows, W), -7.0, dtype=torch.float64 if p.precision == 1 else torch.float32, device=dev)
        it = torch.full((rows, W), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()        # the fills run on torch's stream, the render on the context's own (non-blocking) one
    renderer.render(to_state(fr, p), W, H, fractal_type=fr.FractalType(p.fractal), precision=prec,
                    post_chain=bool(p.post_chain), rgba=rgba, nu=nu, iter=it, shard=shard)
    if host:
        return rgba, nu, it
    return rgba.cpu().numpy(), nu.cpu().numpy(), it.cpu().numpy()


# pixels that passed only through a tolerance EXCEPTION of check_against (the fp32 palette wrap, the pre-gamma comparison
# next to black), against pixels checked: per call the exceptions must stay below EXCEPTION_CAP of the frame, and
# test_tolerance_exceptions_stay_rare (last test of this file) holds the session total to the same cap.
EXCEPTION_CAP = 1e-3
EXCEPTIONS = {"pixels": 0, "wrap": 0, "pre_gamma": 0, "worst_call": 0.0}


def check_against(p, ref_iter, ref_nu, ref_rgba, rgba, nu, it):
    """Holds one render to the bars in this file's header.  Returns the number of pixels that were accepted through a
    tolerance exception (0 for nearly every frame); more than max(2, 0.1 %) of the frame's pixels is a failure, so a
    frame whose colours are systematically off cannot hide behind the exceptions."""
    assert np.array_equal(it, ref_iter), "escape indices differ: %d pixels" % int((it != ref_iter).sum())
    nu = nu.astype(np.float64)
    if p.precision == 1:
        assert np.abs(nu - ref_nu).max() <= NU_TOL_F64
    else:
        ulp = np.spacing(np.maximum(np.abs(ref_nu), 1.0).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(nu - ref_nu) <= 4 * ulp + 4e-6)
    assert np.all(rgba[..., 3] == 1.0)
    d = np.abs(rgba[..., :3] - ref_rgba[..., :3]).max(axis=-1)
    tol = RGB_TOL if not p.post_chain else 1e-4
    if p.precision == 0:
        # fp32: nu itself carries 4 ulp + 4e-6 (v_log_f32 against glibc logf) and reaches the palette multiplied by
        # color_scale / max_iter (palette slope <= ~5): only visible for tiny max_iter (a soak case: max_iter = 1)
        tol += 5.0 * abs(p.color_scale) / p.max_iterations * 8e-6
    bad = d > tol
    n_pre_gamma = n_wrap = 0
    if p.post_chain and bad.any():
        # the chain ends in pow(c, 1/2.2), whose slope is unbounded at 0: a 1e-7 difference of the linear colour next
        # to black (a palette knot evaluated as 0 on one side and 9e-8 on the other) comes out as 3e-4.  Such pixels
        # are compared before the gamma instead.
        lin = np.abs(np.power(rgba[..., :3].astype(np.float64), 2.2) - np.power(ref_rgba[..., :3].astype(np.float64), 2.2)).max(axis=-1)
        n_pre_gamma = int((bad & ~(lin > 1e-6)).sum())
        bad &= lin > 1e-6
    if bad.any():
        assert p.precision == 0 and p.aa <= 1, "colour mismatch %g" % d.max()
        # fp32: tolerate only pixels at the fract() wrap of the palette argument
        scale, off, mi = np.float32(p.color_scale), np.float32(p.color_offset), np.float32(p.max_iterations)
        nu32 = ref_nu.astype(np.float32)
        if p.fractal == 5:      # shaders/test_deep_zoom.comp:86-100: fract(t * k) per palette
            t = (nu32 * scale + off) * np.float32({0: 0.05, 1: 0.03, 2: 0.04}.get(p.palette_mode, 0.02))
        else:
            t = (np.clip(nu32 / mi * scale, 0, 1) + off) if p.fractal == 0 else (off + nu32 / mi * scale)
        u = t - np.floor(t)
        near_wrap = np.minimum(u, 1 - u) < 1e-4
        assert np.all(near_wrap[bad]), "colour mismatch %g away from the palette wrap" % d[bad & ~near_wrap].max()
        n_wrap = int(bad.sum())
    n_exc = n_wrap + n_pre_gamma
    npix = int(d.size)
    EXCEPTIONS["pixels"] += npix
    EXCEPTIONS["wrap"] += n_wrap
    EXCEPTIONS["pre_gamma"] += n_pre_gamma
    EXCEPTIONS["worst_call"] = max(EXCEPTIONS["worst_call"], n_exc / npix)
    assert n_exc <= max(2, EXCEPTION_CAP * npix), \
        "%d of %d pixels needed a tolerance exception (%d palette wrap, %d pre-gamma)" % (n_exc, npix, n_wrap, n_pre_gamma)
    return n_exc


@pytest.mark.parametrize("shape", [3, 4, 6])
@pytest.mark.parametrize("name", sorted(CASES))
def test_case_matches_oracle_and_golden(fr, renderer, oracle, golden, name, shape):
    p, W, H = CASES[name]
    ref = oracle.render(p, W, H)
    g = golden["frames"]
    # the automatic schedule (frames this small take one pass up to max_iter 1536), and the tile pass + lane pool by force
    # wherever it applies (from max_iter 64): both against the oracle and the committed vectors
    for staging in (0, 3):
        renderer.set_tuning(shape=shape)
        renderer.set_option("staging", staging)
        try:
            rgba, nu, it = gpu_render(fr, renderer, p, W, H)
        finally:
            renderer.set_tuning()
            renderer.set_option("staging", 0)
        check_against(p, ref.iter, ref.nu, ref.rgba, rgba, nu, it)
        check_against(p, g[name + "/iter"], g[name + "/nu"], g[name + "/rgba"], rgba, nu, it)


@pytest.mark.parametrize("name", sorted(SPV_CASES))
def test_case_matches_the_executed_reference_shader(fr, renderer, oracle, spv_golden, name):
    """The HIP path (fp32 variants, the arithmetic of the reference's shaders) against what the reference's compiled
    SPIR-V wrote when executed by tests/golden/spirv_interp.py: escape indices bit-exact, texels within the colour bar
    of check_against.  The oracle only supplies the planes the fixture lacks (nu for the wrap exception; SSAA cases)."""
    shader, p, W, H = SPV_CASES[name]
    rgba, nu, it = gpu_render(fr, renderer, p, W, H)
    ref = oracle.render(p, W, H)
    want_iter = spv_golden[name + "/iter"] if p.aa == 1 else ref.iter
    check_against(p, want_iter, ref.nu, spv_golden[name + "/rgba"], rgba, nu, it)


@pytest.mark.parametrize("max_iter", [1, 2, 5, 15, 16, 17, 31, 32, 33, 100])
def test_block_boundaries(fr, renderer, oracle, max_iter):
    """max_iter around the 16-iteration block size of the unchecked fast path."""
    for kw in (dict(), dict(fractal=1, center_x=0.0, julia_c_real=-0.8, julia_c_imag=0.156),
               dict(precision=0), dict(center_x=-0.75, zoom=0.5), dict(fractal=2, center_y=-0.5, zoom=3.5)):
        p = oracle.OracleParams(max_iterations=max_iter, **kw)
        rgba, nu, it = gpu_render(fr, renderer, p, 72, 40)
        ref = oracle.render(p, 72, 40)
        check_against(p, ref.iter, ref.nu, ref.rgba, rgba, nu, it)


def test_optional_planes_and_host_memory(fr, renderer, oracle):
    import torch
    p, W, H = CASES["c2_mandel_f64_mi1024_ragged"]
    ref = oracle.render(p, W, H)
    rgba, nu, it = gpu_render(fr, renderer, p, W, H, host=True)            # FR_MEM_HOST staging path
    check_against(p, ref.iter, ref.nu, ref.rgba, rgba, nu, it)
    st = to_state(fr, p)
    only_nu = torch.empty((H, W), dtype=torch.float64, device="cuda:0")
    renderer.render(st, W, H, nu=only_nu)                                   # a single plane is enough
    assert np.abs(only_nu.cpu().numpy() - ref.nu).max() <= NU_TOL_F64
    only_rgba = np.empty((H, W, 4), np.float32)
    renderer.render(st, W, H, rgba=only_rgba)
    assert np.abs(only_rgba - ref.rgba).max() <= RGB_TOL
    assert renderer.last_kernel_ms() > 0.0


def test_async_on_torch_stream(fr, renderer, oracle):
    import torch
    p, W, H = CASES["seahorse_0008_f64"]
    s = torch.cuda.Stream()
    nu = torch.zeros((H, W), dtype=torch.float64, device="cuda:0")
    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    with torch.cuda.stream(s):
        renderer.render(to_state(fr, p), W, H, rgba=rgba, nu=nu, sync=False, stream=s.cuda_stream)
        doubled = nu * 2            # ordered after the kernel on the same stream
    s.synchronize()
    ref = oracle.render(p, W, H)
    assert np.abs(doubled.cpu().numpy() - 2 * ref.nu).max() <= 2 * NU_TOL_F64
    with pytest.raises(fr.FractalRendererError):
        renderer.render(to_state(fr, p), W, H, rgba=np.empty((H, W, 4), np.float32), sync=False, stream=s.cuda_stream)


@pytest.mark.parametrize("nparts,R", [(2, 1), (2, 5), (3, 8), (8, 4), (8, 64), (5, 7)])
def test_row_strip_shards_reassemble(fr, renderer, oracle, nparts, R):
    p, W, H = CASES["c2_mandel_f64_mi1024_ragged"]
    whole_rgba, whole_nu, whole_it = gpu_render(fr, renderer, p, W, H)
    out_rgba = np.zeros_like(whole_rgba); out_nu = np.zeros_like(whole_nu); out_it = np.zeros_like(whole_it)
    for part in range(nparts):
        sh = fr.Shard(part, nparts, R)
        rows = sh.global_rows(H)
        rgba, nu, it = gpu_render(fr, renderer, p, W, H, shard=sh)
        assert rgba.shape[0] == len(rows)
        if len(rows):
            out_rgba[rows], out_nu[rows], out_it[rows] = rgba, nu, it
    assert np.array_equal(out_it, whole_it) and np.array_equal(out_nu, whole_nu) and np.array_equal(out_rgba, whole_rgba)
    ref = oracle.render(p, W, H)
    check_against(p, ref.iter, ref.nu, ref.rgba, out_rgba, out_nu, out_it)


def test_all_palettes(fr, renderer, oracle):
    for fractal, modes in ((0, MANDEL_PALETTES), (1, JULIA_PALETTES), (2, JULIA_PALETTES)):
        for m in modes:
            p = oracle.OracleParams(fractal=fractal, center_x=0.0 if fractal == 1 else -0.5, palette_mode=m,
                                    max_iterations=96, color_scale=2.5, color_offset=0.1)
            rgba, nu, it = gpu_render(fr, renderer, p, 64, 40)
            ref = oracle.render(p, 64, 40)
            check_against(p, ref.iter, ref.nu, ref.rgba, rgba, nu, it)


# ---- cycle closing in the lane pool ("periodicity") -------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 16, 48, 4096])
@pytest.mark.parametrize("name", sorted(n for n, (p, _, _) in CASES.items()
                                        if p.fractal in (0, 1, 2) and p.aa == 1 and not needs_effects(p) and p.max_iterations >= 128))
def test_periodicity_never_changes_a_pixel(fr, renderer, oracle, name, window):
    """An orbit that returns to its own earlier state can never escape: the lane pool may call it interior
    at once.  Every plane must stay byte-identical to the run without the option, and match the oracle."""
    p, W, H = CASES[name]
    try:
        renderer.set_option("periodicity", -1)       # off: what the reference executes
        base = gpu_render(fr, renderer, p, W, H)
        renderer.set_option("periodicity", window)
        renderer.set_option("staging", 3)            # cycles are closed in the lane-pool pass: run it whatever max_iter is
        cur = gpu_render(fr, renderer, p, W, H)
        assert renderer.last_stages() == 2
        renderer.set_option("staging", 1)            # ... and in the tile kernel of a one-pass frame
        one = gpu_render(fr, renderer, p, W, H)
        assert renderer.last_stages() == 1
    finally:
        renderer.set_option("periodicity", 0)
        renderer.set_option("staging", 0)
    for a, b, c in zip(base, cur, one):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    ref = oracle.render(p, W, H)
    check_against(p, ref.iter, ref.nu, ref.rgba, *cur)


def test_periodicity_on_interior_heavy_views(fr, renderer, oracle):
    """Views that are mostly interior (period 1, 2, 3 components, a period-39 minibrot neighbourhood), shards,
    small refill thresholds: identical planes, and the pass gets shorter where cycles exist."""
    import torch
    views = [dict(center_x=-0.2, center_y=0.0, zoom=0.5, max_iterations=2048),                 # main cardioid, p = 1
             dict(center_x=-1.0, center_y=0.0, zoom=0.6, max_iterations=1500),                 # period-2 disc
             dict(center_x=-0.1225, center_y=0.7449, zoom=0.3, max_iterations=3000),           # period-3 bulb
             dict(center_x=-0.743643887037151, center_y=0.13182590420533, zoom=1e-6, max_iterations=16384),
             dict(fractal=2, center_x=-0.5, center_y=-0.5, zoom=1.0, max_iterations=1024),     # Burning Ship hull
             dict(fractal=1, center_x=0.0, center_y=0.0, zoom=2.0, julia_c_real=-0.12, julia_c_imag=0.74, max_iterations=2000)]
    for kw in views:
        for prec in (1, 0):
            p = oracle.OracleParams(precision=prec, **kw)
            W, H = 320, 200
            try:
                renderer.set_option("periodicity", -1)
                base = gpu_render(fr, renderer, p, W, H)
                for opts in (dict(periodicity=1), dict(periodicity=32, pool_refill_at=1), dict(periodicity=256, pool_refill_at=64),
                             dict(periodicity=1, staging=1),                         # one pass: cycles closed in the tile kernel
                             dict(periodicity=16, staging=1, subtile_shape=4)):      # ... which only exists for 8x8 sub-tiles
                    for k, v in opts.items():
                        renderer.set_option(k, v)
                    cur = gpu_render(fr, renderer, p, W, H)
                    for a, b in zip(base, cur):
                        assert np.array_equal(a, b), (kw, prec, opts)
                    for k in opts:
                        renderer.set_option(k, 0)
                renderer.set_option("periodicity", 1)
                shard = fr.Shard(1, 3, 8)
                part = gpu_render(fr, renderer, p, W, H, shard=shard)
            finally:
                renderer.set_option("periodicity", 0)
                renderer.set_option("pool_refill_at", 0)
            rows = shard.global_rows(H)
            for a, b in zip(base, part):
                assert np.array_equal(a[rows], b)
            assert (base[2] >= p.max_iterations).mean() > 0.2, kw          # the view really is interior-heavy
    # SSAA runs every sample to max_iter in the tile pass: cycles are closed there (escape_run)
    for kw in (dict(center_x=-0.2, zoom=0.5, max_iterations=1500, aa=2), dict(max_iterations=700, aa=3),
               dict(fractal=2, center_x=-0.5, center_y=-0.5, zoom=1.0, max_iterations=600, aa=2, precision=0),
               dict(fractal=1, center_x=0.0, zoom=2.0, julia_c_real=-0.12, julia_c_imag=0.74, max_iterations=900, aa=2)):
        p = oracle.OracleParams(**kw)
        try:
            renderer.set_option("periodicity", -1)
            base = gpu_render(fr, renderer, p, 160, 96)
            for window in (0, 1, 16, 400):
                renderer.set_option("periodicity", window)
                cur = gpu_render(fr, renderer, p, 160, 96)
                for a, b in zip(base, cur):
                    assert np.array_equal(a, b), (kw, window)
        finally:
            renderer.set_option("periodicity", 0)
        ref = oracle.render(p, 160, 96)
        check_against(p, ref.iter, ref.nu, ref.rgba, *base)
    with pytest.raises(fr.FractalRendererError):
        renderer.set_option("periodicity", -2)
    # full size: the C2 frame, byte-identical and faster
    p, W, H = oracle.OracleParams(max_iterations=1024), 4096, 4096
    st = to_state(fr, p)
    planes = {}
    times = {}
    for mode in (-1, 0):                     # off / the default
        renderer.set_option("periodicity", mode)
        try:
            rgba = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
            nu = torch.empty((H, W), dtype=torch.float64, device="cuda:0")
            it = torch.empty((H, W), dtype=torch.int32, device="cuda:0")
            renderer.render(st, W, H, rgba=rgba, nu=nu, iter=it)
            ts = []
            for _ in range(5):
                renderer.render(st, W, H, rgba=rgba)
                ts.append(renderer.last_kernel_ms())
        finally:
            renderer.set_option("periodicity", 0)
        planes[mode] = (rgba, nu, it)
        times[mode] = min(ts)
    for a, b in zip(planes[-1], planes[0]):
        assert torch.equal(a, b)
    assert times[0] < 0.85 * times[-1], times


def test_tuning_variants_are_bit_identical(fr, renderer, oracle):
    """Work-queue geometry and the stage schedule must never change a pixel: every (workgroups/CU, run
    length, sub-tile shape, staging on/off, first budget, budget ratio) gives byte-identical planes."""
    p, W, H = CASES["seahorse_0008_f64"]
    base = gpu_render(fr, renderer, p, 200, 120)
    assert renderer.last_stages() == 1                     # automatic on a frame this small at max_iter 1024: one pass
    renderer.set_option("staging", 3)
    staged_base = gpu_render(fr, renderer, p, 200, 120)
    assert renderer.last_stages() == 2                     # tile pass + lane-pool pass
    renderer.set_option("staging", 0)
    for a, b in zip(base, staged_base):
        assert np.array_equal(a, b)
    opts = ("staging", "stage_first", "stream_run_max", "stream_workgroups_per_cu", "pool_refill_at",
            "probes", "stream_probes", "stream_rotate", "tile_kernel", "tile_pixels", "shards", "regions", "prepare")
    try:
        for wg, run, shape in [(1, 1, 3), (4, 64, 3), (8, 2, 6), (2, 16, 4), (3, 7, 6)]:
            renderer.set_tuning(wg, run, shape)
            renderer.set_option("staging", 3 if wg % 2 else 0)
            cur = gpu_render(fr, renderer, p, 200, 120)
            for a, b in zip(base, cur):
                assert np.array_equal(a, b)
        renderer.set_tuning()
        for kw in (dict(staging=1), dict(stage_first=16), dict(stage_first=64), dict(stage_first=512), dict(stream_run_max=1),
                   dict(probes=8), dict(probes=2), dict(probes=1, stream_probes=1), dict(staging=1, probes=1),
                   dict(probes=3, stream_probes=2), dict(stream_rotate=1), dict(stream_rotate=1, stream_probes=1),
                   dict(stream_rotate=2, stream_probes=8),
                   dict(stage_first=16, stream_workgroups_per_cu=2),
                   dict(staging=3), dict(staging=3, stage_first=64, pool_refill_at=8), dict(staging=3, stage_first=16, pool_refill_at=64),
                   dict(staging=3, stream_run_max=1, stream_workgroups_per_cu=1), dict(staging=3, pool_refill_at=1),
                   # retired schedule selectors (block stages, fused launch) are accepted and select the automatic schedule
                   dict(staging=2), dict(staging=4),
                   # the general tile kernel against the lean one (the default), one and two sub-tiles per trip, 8 and 64
                   # queue shards / stream regions
                   dict(tile_kernel=1), dict(tile_pixels=1), dict(tile_pixels=2, staging=1), dict(tile_pixels=1, staging=1),
                   dict(shards=64), dict(shards=64, regions=8), dict(shards=8, regions=64), dict(shards=64, staging=1),
                   dict(shards=64, tile_kernel=1),
                   dict(shards=64, probes=1, stream_probes=1), dict(shards=64, tile_pixels=1, stream_rotate=1),
                   # control block + coordinate tables in a launch of their own instead of the tile pass's prologue
                   dict(prepare=1), dict(prepare=1, staging=1), dict(prepare=1, shards=64, tile_pixels=1)):
            if "staging" not in kw:
                kw = dict(kw, staging=3)               # (the automatic choice for a frame this small is one pass)
            for k, v in kw.items():
                renderer.set_option(k, v)
            cur = gpu_render(fr, renderer, p, 200, 120)
            assert (renderer.last_stages() > 1) == (kw["staging"] == 3)     # (2 and 4, retired, select the automatic schedule)
            for a, b in zip(base, cur):
                assert np.array_equal(a, b), kw
            for k in opts:
                renderer.set_option(k, 0)
    finally:
        renderer.set_tuning()
        for k in opts:
            renderer.set_option(k, 0)


def test_mandelbrot_effects_through_the_lean_kernels_equal_the_effects_variant(fr, renderer):
    """The Mandelbrot shader's effects need nothing along the orbit.  Stripe shading reads the z of a sample's last update; the
    orbit trap's minimum is the constant 0 as the shader is written (z = c exactly after the first update, and length(z - c) is
    part of the minimum: shaders/mandelbrot.comp:153-166), so the trap blend is a constant mix and the trap-coloured interior
    a constant colour.  Such frames take the lean tile pass and the lane pool in their code-3 instantiations (shade_stripes:
    the pool keeps every finished lane's z and, where a striped interior reads it, lets no stretch cross a deadline) instead
    of the effects variant's lockstep run with four running minima.  Both routes must give the same planes bit for bit:
    stripes alone / with the orbit trap / the trap alone / the trap-coloured interior, fp64 / fp32, one pass and two, post
    chain, ragged frames, row strips, supersampled, every pool tuning that moves deadlines and stretches around."""
    import torch
    views = [dict(max_iterations=1024), dict(max_iterations=700, center_x=-0.743643887037151, center_y=0.13182590420533, zoom=0.02),
             dict(max_iterations=300, zoom=1.5), dict(max_iterations=2000, center_x=-0.1011, center_y=0.9563, zoom=0.05)]
    opts = ("stripes", "staging", "stage_first", "pool_refill_at", "tile_exit", "tile_exit_from", "shards", "prepare", "stream_run_max")
    tunes = (dict(), dict(staging=1), dict(staging=3, stage_first=32), dict(staging=3, stage_first=160, pool_refill_at=1),
             dict(staging=3, pool_refill_at=64, tile_exit=2, tile_exit_from=16), dict(staging=3, shards=64, prepare=1),
             dict(staging=3, stage_first=48, stream_run_max=4))

    def planes(rows, W, nu_dt):
        out = (torch.full((rows, W, 4), -1.0, dtype=torch.float32, device="cuda"), torch.full((rows, W), -1.0, dtype=nu_dt, device="cuda"),
               torch.full((rows, W), -1, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        return out

    try:
        for k, kw in enumerate(views):
            for prec in (fr.Precision.F64, fr.Precision.F32):
                nu_dt = torch.float64 if prec == fr.Precision.F64 else torch.float32
                for combo in range(4):
                    eff = (dict(stripe_enabled=True, interior_style=k % 2),
                           dict(stripe_enabled=True, orbit_trap_enabled=True, interior_style=k % 2),
                           dict(orbit_trap_enabled=True, orbit_trap_radius=0.2 + 0.3 * k, interior_style=(k + 1) % 2),
                           dict(interior_style=2, orbit_trap_radius=0.1 + 0.2 * k, stripe_enabled=bool(k % 2)))[combo]
                    st = fr.FractalState(stripe_density=(3.0, 7.5, 12.0, 20.0)[k], color_offset=0.1 * k, color_scale=1.0 + k,
                                         palette_mode=k % 6, **eff, **kw)
                    for W, H in ((264, 152), (131, 67))[:2 if combo == 0 else 1]:
                        def run(shard=None, rows=H, post=False, **tune):
                            for o in opts:
                                renderer.set_option(o, tune.get(o, 0))
                            out = planes(rows, W, nu_dt)
                            renderer.render(st, W, H, precision=prec, post_chain=post, rgba=out[0], nu=out[1], iter=out[2], shard=shard)
                            return out
                        for post in (False, True):
                            want = run(post=post, stripes=1)
                            assert renderer.last_stages() == 1                    # the effects variant: one lockstep pass
                            for tune in (tunes if combo == 0 else tunes[:3]):
                                got = run(post=post, **tune)
                                for a, b in zip(want, got):
                                    assert torch.equal(a, b), (k, prec, combo, W, H, post, tune)
                        sh = fr.Shard(1, 3, 16)
                        w2, g2 = run(sh, sh.rows(H), stripes=1), run(sh, sh.rows(H), staging=3)
                        for a, b in zip(w2, g2):
                            assert torch.equal(a, b), (k, prec, combo, W, H, "strips")
                    # supersampled: the sample loop of the effects variant against the staged sample grid in the code-3 instantiations
                    st_aa = fr.FractalState(stripe_density=(3.0, 7.5, 12.0, 20.0)[k], antialiasing_samples=2 + k % 2, palette_mode=k % 6,
                                            **eff, **kw)
                    W, H = 136, 72
                    outs = []
                    for stripes in (1, 0):
                        for o in opts:
                            renderer.set_option(o, 0)
                        renderer.set_option("stripes", stripes)
                        out = planes(H, W, nu_dt)
                        renderer.render(st_aa, W, H, precision=prec, post_chain=bool(k % 2), rgba=out[0], nu=out[1], iter=out[2])
                        outs.append(out)
                    for a, b in zip(*outs):
                        assert torch.equal(a, b), (k, prec, combo, "ssaa")
    finally:
        for o in opts:
            renderer.set_option(o, 0)


@pytest.mark.parametrize("name", ["seahorse_0008_f64", "c3_julia_f32_centre0", "ship_f64_ragged_mi2048", "c2_mandel_f64_mi1024_ragged"])
def test_occupancy_exit_of_the_tile_pass_is_bit_identical(fr, renderer, oracle, name):
    """A trip of the lean tile pass whose live samples are few hands them to the lane pool before its budget b0 is spent
    (escape_run_lean, "tile_exit" = the assumed per-record cost of the pool in updates, "tile_exit_from" = not before): the
    records then carry different update counts, the pool honours each (deadlines, deferred escapes, cycle closing).  Off
    ("tile_exit" = 1) against: the automatic rule, a rule that leaves as soon as one sample has finished (cost 2, from 16:
    nearly every record leaves early), one that never fires (4096) -- with and without cycle closing, two budgets, ragged
    frames, and the general tile kernel as the independent side."""
    p = CASES[name][0]
    opts = ("tile_kernel", "tile_exit", "tile_exit_from", "periodicity", "stage_first", "staging", "pool_refill_at")
    try:
        for W, H in ((200, 120), (264, 40), (17, 64)):
            renderer.set_option("staging", 3)
            renderer.set_option("tile_kernel", 1)
            base = gpu_render(fr, renderer, p, W, H)
            renderer.set_option("tile_kernel", 0)
            for kw in (dict(tile_exit=1), dict(), dict(tile_exit=2, tile_exit_from=16), dict(tile_exit=2, tile_exit_from=16, periodicity=1),
                       dict(tile_exit=2, tile_exit_from=16, periodicity=-1), dict(tile_exit=8, tile_exit_from=32, stage_first=64),
                       dict(tile_exit=8, tile_exit_from=16, stage_first=160, periodicity=1), dict(tile_exit=4096),
                       dict(tile_exit=48, tile_exit_from=48, periodicity=-1), dict(tile_exit=2, tile_exit_from=16, pool_refill_at=1),
                       dict(tile_exit=3, tile_exit_from=1, stage_first=48, pool_refill_at=64, periodicity=1)):
                for k in opts[1:]:
                    if k != "staging":
                        renderer.set_option(k, kw.get(k, 0))
                cur = gpu_render(fr, renderer, p, W, H)
                assert renderer.last_stages() == 2
                for a, b in zip(base, cur):
                    assert np.array_equal(a, b), (W, H, kw)
    finally:
        for k in opts:
            renderer.set_option(k, 0)


@pytest.mark.parametrize("name", ["seahorse_0008_f64", "c3_julia_f32_centre0", "ship_f64_ragged_mi2048", "julia_c_outside_bailout"])
def test_lean_tile_kernel_equals_the_general_one(fr, renderer, oracle, name):
    """tile_lean_kernel (coordinate tables, NaN-threshold parking, two sub-tiles per trip) against tile_kernel, and 64
    queue shards / stream regions against 8: byte-identical planes on ragged sizes (odd numbers of sub-tiles per row:
    trips whose second sub-tile does not exist), one-pass and staged, whole frames and row-strip shards whose strips are
    whole sub-tile rows (the lean kernel's condition; other strip heights take the general kernel)."""
    p, _, _ = CASES[name]
    opts = ("tile_kernel", "tile_pixels", "shards", "regions", "staging", "periodicity")
    try:
        for W, H in ((200, 120), (9, 9), (136, 8), (17, 64), (1, 1), (264, 40)):
            for staging in (0, 1):
                renderer.set_option("staging", staging)
                renderer.set_option("tile_kernel", 1)
                renderer.set_option("shards", 8)
                base = gpu_render(fr, renderer, p, W, H)
                for kw in (dict(), dict(tile_pixels=1), dict(shards=64), dict(shards=64, tile_pixels=1), dict(periodicity=-1),
                           dict(shards=64, regions=8)):
                    renderer.set_option("tile_kernel", 0)
                    for k in ("tile_pixels", "shards", "regions", "periodicity"):
                        renderer.set_option(k, kw.get(k, 0))
                    cur = gpu_render(fr, renderer, p, W, H)
                    for a, b in zip(base, cur):
                        assert np.array_equal(a, b), (W, H, staging, kw)
        # row strips: 8 and 16 rows per strip run the lean kernel, 4 the general one
        renderer.set_option("staging", 0)
        for k in ("tile_pixels", "shards", "regions", "periodicity"):
            renderer.set_option(k, 0)
        W, H = 200, 120
        whole = gpu_render(fr, renderer, p, W, H)
        for nparts, R in ((2, 8), (3, 16), (2, 4)):
            for part in range(nparts):
                sh = fr.Shard(part, nparts, R)
                rows = sh.global_rows(H)
                for shards in (0, 64):
                    renderer.set_option("shards", shards)
                    got = gpu_render(fr, renderer, p, W, H, shard=sh)
                    for a, b in zip(whole, got):
                        assert np.array_equal(a[rows], b), (nparts, R, part, shards)
    finally:
        for k in opts:
            renderer.set_option(k, 0)


@pytest.mark.parametrize("refill_at", [1, 7, 32, 64])
@pytest.mark.parametrize("name", sorted(n for n, (p, _, _) in CASES.items()
                                         if p.fractal <= 2 and p.aa <= 1 and not needs_effects(p)))
def test_lane_pool_matches_oracle(fr, renderer, oracle, name, refill_at):
    """The lane pool (lanes refilled with the next survivor record as they finish), whatever its refill threshold and
    with a short tile pass in front of it so that most samples reach it, against the oracle and, bitwise, against the
    single pass."""
    p, W, H = CASES[name]
    try:
        renderer.set_option("staging", 1)
        tile = gpu_render(fr, renderer, p, W, H)
        renderer.set_option("staging", 3)
        renderer.set_option("stage_first", 16)
        renderer.set_option("pool_refill_at", refill_at)
        rgba, nu, it = gpu_render(fr, renderer, p, W, H)
        assert renderer.last_stages() == (2 if p.max_iterations >= 32 else 1)
    finally:
        renderer.set_option("stage_first", 0)
        renderer.set_option("pool_refill_at", 0)
        renderer.set_option("staging", 0)
    ref = oracle.render(p, W, H)
    check_against(p, ref.iter, ref.nu, ref.rgba, rgba, nu, it)
    for a, b in zip(tile, (rgba, nu, it)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["c3_julia_f32_centre0", "c2_mandel_f64_mi1024_ragged", "c4_seahorse_deep_f64", "mandel_small_bailout",
                                  "ship_f32_the_ship"])
def test_lane_pool_larger_frames_and_shards(fr, renderer, oracle, name):
    p, _, _ = CASES[name]
    W, H = 333, 207
    try:
        renderer.set_option("staging", 1)
        tile = gpu_render(fr, renderer, p, W, H)
        tile_sh = gpu_render(fr, renderer, p, W, H, shard=fr.Shard(1, 3, 8))
        renderer.set_option("staging", 3)
        for shape in (3, 6, 4):
            renderer.set_tuning(shape=shape)
            pool = gpu_render(fr, renderer, p, W, H)
            assert renderer.last_stages() == 2
            for a, b in zip(tile, pool):
                assert np.array_equal(a, b)
        renderer.set_tuning()
        pool_sh = gpu_render(fr, renderer, p, W, H, shard=fr.Shard(1, 3, 8))
        for a, b in zip(tile_sh, pool_sh):
            assert np.array_equal(a, b)
    finally:
        renderer.set_option("staging", 0)
        renderer.set_tuning()


@pytest.mark.parametrize("name", ["c3_julia_f32_centre0", "julia_f64_default_c", "c2_mandel_f32_mi1024",
                                  "c4_seahorse_deep_f64", "mandel_small_bailout", "mandel_big_bailout",
                                  "julia_c_outside_bailout", "mandel_scale_offset", "ship_f32_the_ship",
                                  "ship_f64_ragged_mi2048", "ship_small_bailout_f64"])
def test_staged_equals_single_pass(fr, renderer, oracle, name):
    """Survivor compaction (tile pass + lane-pool pass) against the single-pass kernel, bitwise, on a
    frame large enough that rings wrap and blocks are partially filled."""
    p, _, _ = CASES[name]
    W, H = 333, 207
    try:
        renderer.set_option("staging", 1)
        single = gpu_render(fr, renderer, p, W, H)
        assert renderer.last_stages() == 1
    finally:
        renderer.set_option("staging", 0)
    for mode in (3, 0):                    # 3: tile pass + one lane-pool pass over the survivors whatever max_iter is
        try:
            renderer.set_option("staging", mode)
            staged = gpu_render(fr, renderer, p, W, H)
            n = renderer.last_stages()
        finally:
            renderer.set_option("staging", 0)
        # automatic (0) on a frame of 69 000 pixels: two passes from max_iter 1536 on (Julia: 256), else one; forced: from 2 budgets on
        assert n > 1 or p.max_iterations < ((256 if p.fractal == 1 else 1536) if mode == 0 else 64), (mode, n)
        for a, b in zip(staged, single):
            assert np.array_equal(a, b), mode


def test_two_pass_schedule_under_every_geometry(fr, renderer, oracle):
    """Queue geometry, refill threshold, tile-pass budget, cycle closing and row-strip shards must not change a pixel of
    the tile pass + lane-pool schedule."""
    for name in ("seahorse_0008_f64", "c3_julia_f32_centre0", "ship_f64_ragged_mi2048", "reset_view_f64"):
        p, _, _ = CASES[name]
        W, H = 280, 168
        try:
            renderer.set_option("staging", 1)
            base = gpu_render(fr, renderer, p, W, H)
            base_sh = gpu_render(fr, renderer, p, W, H, shard=fr.Shard(2, 3, 8))
            renderer.set_option("staging", 3)
            for kw in (dict(), dict(workgroups_per_cu=1), dict(workgroups_per_cu=8, run_max=1), dict(run_max=64, run_min=16),
                       dict(pool_refill_at=1), dict(pool_refill_at=64), dict(stage_first=16), dict(stage_first=48, pool_refill_at=7),
                       dict(probes=1), dict(probes=3, run_max=2), dict(periodicity=1), dict(periodicity=16, pool_refill_at=3),
                       dict(periodicity=4096), dict(shift_bias=-4), dict(shift_bias=6), dict(stream_workgroups_per_cu=1),
                       dict(stream_run_max=8, stream_run_min=4), dict(regions=64), dict(stream_rotate=1, stream_probes=1)):
                for k, v in kw.items():
                    renderer.set_option(k, v)
                cur = gpu_render(fr, renderer, p, W, H)
                assert renderer.last_stages() == 2
                for a, b in zip(base, cur):
                    assert np.array_equal(a, b), (name, kw)
                part = gpu_render(fr, renderer, p, W, H, shard=fr.Shard(2, 3, 8))
                for a, b in zip(base_sh, part):
                    assert np.array_equal(a, b), (name, kw)
                for k in kw:
                    renderer.set_option(k, 0)
        finally:
            for k in ("staging", "workgroups_per_cu", "run_max", "run_min", "pool_refill_at", "stage_first", "probes",
                      "periodicity", "shift_bias", "stream_workgroups_per_cu", "stream_run_max", "stream_run_min", "regions",
                      "stream_rotate", "stream_probes"):
                renderer.set_option(k, 0)


def test_export_rgb8(fr, renderer, oracle):
    """fr_export_rgb8 against the restated CPU loop of src/vk_engine.cpp:1344-1371: the BYTES are identical (the kernel's
    fast gamma estimate is corrected against the powf thresholds, fr_export8_thresholds) -- on a rendered frame, on random
    planes (out-of-range, negative and huge values included), on planes whose values sit within a few ulps of every
    truncation edge, for widths that take the four-pixel and the one-pixel form, with and without the fp16 rounding."""
    import torch
    p, W, H = CASES["c1_mandel_f64_default"]
    rgba, _, _ = gpu_render(fr, renderer, p, W, H)
    rng = np.random.default_rng(8)
    planes = [rgba]
    for (h, w) in ((37, 64), (20, 61), (5, 1), (64, 256)):
        x = rng.random((h, w, 4), dtype=np.float32)
        x[..., :3] *= rng.choice(np.array([1.0, 1.0, 0.05, 3.0, 40.0], np.float32), size=(h, w, 3))
        x[rng.random((h, w)) < 0.02] = -0.25
        planes.append(np.ascontiguousarray(x))
    # values next to every truncation edge: a = t[b] moved by -3..+3 ulps, pulled back through the tonemap
    # (x = the root of aces(x) = a, refined in double), then x itself moved by -2..+2 ulps
    t = np.array(fr.export8_thresholds()[1:256], np.float32)
    a = (t.view(np.uint32)[:, None] + np.arange(-3, 4, dtype=np.int64)[None, :]).astype(np.uint32).view(np.float32).astype(np.float64)
    a = np.clip(a, 0.0, 0.999)
    # aces(x) = (x (2.51 x + 0.03)) / (x (2.43 x + 0.59) + 0.14) = a  ->  (2.51 - 2.43 a) x^2 + (0.03 - 0.59 a) x - 0.14 a = 0
    qa, qb, qc = 2.51 - 2.43 * a, 0.03 - 0.59 * a, -0.14 * a
    x = ((-qb + np.sqrt(qb * qb - 4 * qa * qc)) / (2 * qa)).astype(np.float32)
    xs = (x.view(np.uint32)[..., None].astype(np.int64) + np.arange(-2, 3, dtype=np.int64)).astype(np.uint32).view(np.float32).ravel()
    n4 = (xs.size + 11) // 12 * 12
    edge = np.zeros(n4, np.float32); edge[:xs.size] = xs
    edge_plane = np.ones((n4 // 12, 4, 4), np.float32)
    edge_plane[..., :3] = edge.reshape(n4 // 12, 4, 3)
    planes.append(edge_plane)
    for src in planes:
        h, w = src.shape[:2]
        for through_half in (False, True):
            got = renderer.export_rgb8(src, w, h, through_half=through_half)
            ref = oracle.export_rgb8(src, through_half=through_half)
            assert np.array_equal(got, ref), (src.shape, through_half, int((got != ref).sum()))
    dev = torch.from_numpy(rgba).cuda()
    out = renderer.export_rgb8(dev, W, H)
    assert out.is_cuda and np.array_equal(out.cpu().numpy(), renderer.export_rgb8(rgba, W, H))
    # an output pointer at an odd byte offset (a caller's sub-buffer): the one-pixel form, same bytes
    big = torch.zeros(W * H * 3 + 8, dtype=torch.uint8, device="cuda")
    for off in (1, 2, 4):
        view = big[off:off + W * H * 3].view(H, W, 3)
        renderer.export_rgb8(dev, W, H, out=view)
        assert torch.equal(view, out), off
    big16 = torch.zeros(W * H * 3 + 8, dtype=torch.int16, device="cuda")
    ref16 = renderer.export_rgb16(dev, W, H)
    for off in (1, 2, 3):
        view = big16[off:off + W * H * 3].view(H, W, 3)
        renderer.export_rgb16(dev, W, H, out=view)
        assert torch.equal(view, ref16), off


def test_export_rgb8_full_size_plane_is_byte_exact(fr, renderer, oracle):
    """A 4096^2 post-chained C2 frame (50 M channel values) through fr_export_rgb8 with the fp16 rounding of the
    reference's storage image: identical to the restated CPU loop, byte for byte."""
    import torch
    W = H = 4096
    rgba = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    renderer.render(fr.FractalState(max_iterations=1024), W, H, rgba=rgba, post_chain=True)
    got = renderer.export_rgb8(rgba, W, H, through_half=True).cpu().numpy()
    ref = oracle.export_rgb8(rgba.cpu().numpy(), through_half=True)
    assert np.array_equal(got, ref), int((got != ref).sum())


def test_render_errors(fr, renderer):
    st = fr.FractalState()
    buf = np.empty((8, 8, 4), np.float32)
    with pytest.raises(fr.FractalRendererError) as e:
        renderer.render(st, 8, 8, fractal_type=fr.FractalType.Phoenix, rgba=buf)
    assert e.value.status == fr._capi.FR_ERR_UNSUPPORTED
    with pytest.raises(fr.FractalRendererError):
        renderer.render(fr.FractalState(max_iterations=0), 8, 8, rgba=buf)
    with pytest.raises(fr.FractalRendererError):
        renderer.render(st, 8, 8)                                  # no plane at all
    with pytest.raises(ValueError):
        renderer.render(st, 8, 8, rgba=np.empty((8, 8, 3), np.float32))
    with pytest.raises(fr.FractalRendererError) as e:
        fr.Renderer(99)
    assert e.value.status == fr._capi.FR_ERR_NO_DEVICE


# ---- BASELINE.json sizes: size-independent properties ---------------------------------------------------------------
def test_c2_full_size_properties(fr, renderer, oracle):
    """Mandelbrot 4096x4096, max_iter 1024, fp64 (the metric's configuration)."""
    import torch
    W = H = 4096
    p = oracle.OracleParams(max_iterations=1024)
    dev = torch.device("cuda:0")
    rgba = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    nu = torch.empty((H, W), dtype=torch.float64, device=dev)
    it = torch.empty((H, W), dtype=torch.int32, device=dev)
    renderer.render(to_state(fr, p), W, H, rgba=rgba, nu=nu, iter=it)
    # (1) conjugate symmetry: centre_y = 0, so rows y and H-y hold c and conj(c) exactly
    assert torch.equal(it[1:], it[1:].flip(0)) and torch.equal(nu[1:], nu[1:].flip(0))
    assert torch.equal(rgba[1:], rgba[1:].flip(0))
    # (2) sampled rows against the oracle (full width, so every sub-tile column is covered)
    for y0 in (0, 1000, 2040, 2048, 3333, 4088):
        ref = oracle.render(p, W, H, y0=y0, y1=y0 + 8)
        check_against(p, ref.iter, ref.nu, ref.rgba, rgba[y0:y0 + 8].cpu().numpy(), nu[y0:y0 + 8].cpu().numpy(),
                      it[y0:y0 + 8].cpu().numpy())
    # (3) interior fraction / mean iterations match the survey's workload table
    it_h = it.cpu().numpy()
    interior = float((it_h == 1024).mean())
    mean_it = float(np.where(it_h < 1024, it_h.astype(np.int64) + 1, 1024).mean())
    assert abs(interior - 0.168) < 0.003 and abs(mean_it - 177.9) < 1.0
    # (4) checksum of checksums is independent of the queue geometry and of row-strip sharding
    want = (int(it.to(torch.int64).sum()), float(nu.sum()), float(rgba.double().sum()))
    try:
        renderer.set_tuning(4, 3, 6)
        nu2 = torch.empty_like(nu); it2 = torch.empty_like(it); rgba2 = torch.empty_like(rgba)
        renderer.render(to_state(fr, p), W, H, rgba=rgba2, nu=nu2, iter=it2)
        assert torch.equal(it2, it) and torch.equal(nu2, nu) and torch.equal(rgba2, rgba)
        renderer.set_tuning()
        renderer.set_option("stage_first", 256)    # a long tile pass in front of the lane pool at full size
        renderer.render(to_state(fr, p), W, H, rgba=rgba2, nu=nu2, iter=it2)
        assert renderer.last_stages() == 2
        assert torch.equal(it2, it) and torch.equal(nu2, nu) and torch.equal(rgba2, rgba)
        renderer.set_option("stage_first", 0)
        renderer.set_option("staging", 1)          # single pass
        renderer.render(to_state(fr, p), W, H, rgba=rgba2, nu=nu2, iter=it2)
        assert renderer.last_stages() == 1
        assert torch.equal(it2, it) and torch.equal(nu2, nu) and torch.equal(rgba2, rgba)
        renderer.set_option("staging", 0)
        # the general tile kernel / 8 shards and regions / one sub-tile per trip against the defaults (lean, 64, two)
        for kw in (dict(tile_kernel=1), dict(shards=8), dict(tile_pixels=1), dict(shards=64, regions=8), dict(tile_kernel=1, shards=8)):
            for k, v in kw.items():
                renderer.set_option(k, v)
            renderer.render(to_state(fr, p), W, H, rgba=rgba2, nu=nu2, iter=it2)
            assert torch.equal(it2, it) and torch.equal(nu2, nu) and torch.equal(rgba2, rgba), kw
            for k in kw:
                renderer.set_option(k, 0)
    finally:
        renderer.set_tuning()
        for k in ("staging", "stage_first", "tile_kernel", "shards", "regions", "tile_pixels"):
            renderer.set_option(k, 0)
    tot_it, tot_nu = 0, 0.0
    for part in range(8):
        sh = fr.Shard(part, 8, 32)
        n = sh.rows(H)
        nus = torch.empty((n, W), dtype=torch.float64, device=dev); its = torch.empty((n, W), dtype=torch.int32, device=dev)
        renderer.render(to_state(fr, p), W, H, nu=nus, iter=its, shard=sh)
        rows = torch.from_numpy(sh.global_rows(H)).to(dev)
        assert torch.equal(its, it[rows]) and torch.equal(nus, nu[rows])
        tot_it += int(its.to(torch.int64).sum())
    assert tot_it == want[0]


def test_c3_julia_full_size_rows(fr, renderer, oracle):
    """Julia c = -0.8+0.156i, 4096x4096, max_iter 2048, fp32."""
    import torch
    W = H = 4096
    p = oracle.OracleParams(fractal=1, precision=0, center_x=0.0, center_y=0.0, zoom=3.0, max_iterations=2048,
                            julia_c_real=-0.8, julia_c_imag=0.156)
    dev = torch.device("cuda:0")
    rgba = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    nu = torch.empty((H, W), dtype=torch.float32, device=dev)
    it = torch.empty((H, W), dtype=torch.int32, device=dev)
    renderer.render(to_state(fr, p), W, H, fractal_type=fr.FractalType.JuliaSet, precision=fr.Precision.F32,
                    rgba=rgba, nu=nu, iter=it)
    for y0 in (0, 1024, 2044, 2048, 4090):
        y1 = min(H, y0 + 6)
        ref = oracle.render(p, W, H, y0=y0, y1=y1)
        check_against(p, ref.iter, ref.nu, ref.rgba, rgba[y0:y1].cpu().numpy(), nu[y0:y1].cpu().numpy(), it[y0:y1].cpu().numpy())
    # point symmetry of a Julia set about the view centre: pixel (x,y) <-> (W-x, H-y) map to z0 and -z0
    assert torch.equal(it[1:, 1:], it[1:, 1:].flip(0, 1))


def test_c4_deep_zoom_window(fr, renderer, oracle):
    """C4 view (Seahorse, zoom 1e-6, max_iter 16384, fp64) on a window the oracle finishes in seconds;
    the 8192^2 frame's pixel pitch is kept by rendering a 8192-high frame's row band."""
    p, W, H = CASES["c4_seahorse_deep_f64"]
    p = type(p)(**{**p.__dict__})
    W, H = 512, 8192
    sh = fr.Shard(16, 64, 8)            # strips of 8 rows: this part = rows 128..135, 640..647, ... (128 rows)
    rows = sh.global_rows(H)[:24]
    rgba, nu, it = gpu_render(fr, renderer, p, W, H, shard=sh)
    for r0 in (0, 8, 16):
        y0 = int(rows[r0])
        ref = oracle.render(p, W, H, y0=y0, y1=y0 + 8)
        check_against(p, ref.iter, ref.nu, ref.rgba, rgba[r0:r0 + 8], nu[r0:r0 + 8], it[r0:r0 + 8])


def test_c5_franim_frames(fr, renderer, oracle, golden):
    """C5: frames of the reference's sample .franim (t = frame / target_fps), max_iter override 4096,
    row strips dealt to 8 parts; one part of each sampled frame is checked against the oracle."""
    a = fr.AnimationSystem()
    assert a.load_from_file(golden["franim"])
    W, H = 512, 512
    for frame in (0, 300, 599, 1234, 2399):
        st = a.interpolate(a.frame_time(frame))
        st.max_iterations = 4096
        sh = fr.Shard(frame % 8, 8, 16)
        rows = sh.global_rows(H)
        p = oracle.OracleParams(center_x=st.center_x, center_y=st.center_y, zoom=st.zoom, max_iterations=4096,
                                palette_mode=st.palette_mode, color_offset=st.color_offset, color_scale=st.color_scale)
        rgba, nu, it = gpu_render(fr, renderer, p, W, H, shard=sh)
        y0 = int(rows[16])
        ref = oracle.render(p, W, H, y0=y0, y1=y0 + 16)
        check_against(p, ref.iter, ref.nu, ref.rgba, rgba[16:32], nu[16:32], it[16:32])


def test_c1_full_size(fr, renderer, oracle):
    """C1 (BASELINE.json configs[0]): Mandelbrot 512x512, max_iter 256, fp64, default viewport -- the whole frame
    against the oracle, the workload table of BASELINE.md section 4, conjugate symmetry, and the host-buffer path."""
    W = H = 512
    p = oracle.OracleParams(max_iterations=256)
    ref = oracle.render(p, W, H)
    rgba, nu, it = gpu_render(fr, renderer, p, W, H)
    assert renderer.last_stages() == 1                      # below the staging threshold: one pass
    check_against(p, ref.iter, ref.nu, ref.rgba, rgba, nu, it)
    assert np.array_equal(it[1:], it[1:][::-1]) and np.array_equal(nu[1:], nu[1:][::-1])
    interior = float((it == 256).mean())
    mean_it = float(np.where(it < 256, it.astype(np.int64) + 1, 256).mean())
    assert abs(interior - 0.169) < 0.003 and abs(mean_it - 48.5) < 0.5, (interior, mean_it)
    host = gpu_render(fr, renderer, p, W, H, host=True)
    for a, b in zip((rgba, nu, it), host):
        assert np.array_equal(a, b)
    try:                                                    # the two-pass schedule on the same frame
        renderer.set_option("staging", 3)
        two = gpu_render(fr, renderer, p, W, H)
        assert renderer.last_stages() == 2
    finally:
        renderer.set_option("staging", 0)
    for a, b in zip((rgba, nu, it), two):
        assert np.array_equal(a, b)


def _band_check(oracle, p, W, H, planes, bands, rows=4):
    """sampled full-width row bands of device planes (rgba, nu, it) against the oracle"""
    rgba, nu, it = planes
    for y0 in bands:
        y1 = min(H, y0 + rows)
        ref = oracle.render(p, W, H, y0=y0, y1=y1)
        check_against(p, ref.iter, ref.nu, ref.rgba, rgba[y0:y1].cpu().numpy(), nu[y0:y1].cpu().numpy(), it[y0:y1].cpu().numpy())


def test_c4_full_size(fr, renderer, oracle):
    """C4 (BASELINE.json configs[3]) AS STATED: Mandelbrot 8192x8192, max_iter 16384, fp64, Seahorse deep preset at
    zoom 1e-6.  Sampled full-width row bands against the oracle; interior fraction / mean iterations against
    BASELINE.md section 4 (74.7 %, 12 553.6); every plane byte-identical under cycle closing on / off, the single
    pass, and as 8 row bands and 8-way interleaved strips."""
    import torch
    W = H = 8192
    p = oracle.OracleParams(center_x=-0.743643887037151, center_y=0.13182590420533, zoom=1e-6, max_iterations=16384)
    st = to_state(fr, p)
    dev = torch.device("cuda:0")
    mk = lambda rows: (torch.empty((rows, W, 4), dtype=torch.float32, device=dev),       # noqa: E731
                       torch.empty((rows, W), dtype=torch.float64, device=dev),
                       torch.empty((rows, W), dtype=torch.int32, device=dev))
    base = mk(H)
    try:
        renderer.set_option("periodicity", -1)                           # off: every interior sample runs its 16384 updates
        renderer.render(st, W, H, rgba=base[0], nu=base[1], iter=base[2])
        assert renderer.last_stages() == 2
        t_plain = renderer.last_kernel_ms()
        _band_check(oracle, p, W, H, base, (0, 2731, 4094, 8188))
        it = base[2]
        interior = float((it == 16384).double().mean())
        mean_it = float(torch.where(it < 16384, it.to(torch.int64) + 1, torch.full_like(it, 16384, dtype=torch.int64)).double().mean())
        assert abs(interior - 0.747) < 0.003 and abs(mean_it - 12555.0) < 30.0, (interior, mean_it)
        other = mk(H)
        for opts in (dict(periodicity=0), dict(periodicity=-1, staging=1)):
            for k, v in opts.items():
                renderer.set_option(k, v)
            for t in other:
                t.fill_(-3)
            torch.cuda.synchronize()     # torch's stream and the context's stream are not ordered with each other
            renderer.render(st, W, H, rgba=other[0], nu=other[1], iter=other[2])
            for a, b in zip(base, other):
                assert torch.equal(a, b), opts
            if opts["periodicity"] == 0:
                assert renderer.last_kernel_ms() < 0.85 * t_plain        # the interior runs are cut short
            renderer.set_option("staging", 0)
        del other
        renderer.set_option("periodicity", 1)                            # shards: with cycle closing (3x faster here)
        for layout_R in (H // 8, 32):                                    # 8 contiguous row bands; interleaved strips of 32
            for part in range(8):
                sh = fr.Shard(part, 8, layout_R)
                n = sh.rows(H)
                got = mk(n)
                renderer.render(st, W, H, rgba=got[0], nu=got[1], iter=got[2], shard=sh)
                rows = torch.from_numpy(sh.global_rows(H)).to(dev)
                for a, b in zip(base, got):
                    assert torch.equal(a[rows], b), (layout_R, part)
                del got
    finally:
        renderer.set_option("periodicity", 0)
        renderer.set_option("staging", 0)


def test_c5_full_size_row_bands(fr, renderer, oracle, golden):
    """C5 (BASELINE.json configs[4]) AS STATED on one card: 8192x8192, max_iter 4096 (override), fp64, frames of the
    reference's sample .franim at t = frame / target_fps, each rendered as the 8 disjoint row bands the 8 ranks would
    render (rotating over the frame index as FrameExchange does), assembled, and compared -- bitwise with the
    whole-frame render, and on sampled full-width row bands with the oracle.  The ranks' RCCL exchange itself is
    covered by the gloo tests and the two-rank rehearsal; this is the arithmetic at the stated size."""
    import torch
    W = H = 8192
    a = fr.AnimationSystem()
    assert a.load_from_file(golden["franim"])
    dev = torch.device("cuda:0")
    for frame in (1234, 2399):
        st = a.interpolate(a.frame_time(frame))
        st.max_iterations = 4096
        p = oracle.OracleParams(center_x=st.center_x, center_y=st.center_y, zoom=st.zoom, max_iterations=4096,
                                palette_mode=st.palette_mode, color_offset=st.color_offset, color_scale=st.color_scale)
        whole = (torch.empty((H, W, 4), dtype=torch.float32, device=dev), torch.empty((H, W), dtype=torch.float64, device=dev),
                 torch.empty((H, W), dtype=torch.int32, device=dev))
        renderer.render(st, W, H, rgba=whole[0], nu=whole[1], iter=whole[2])
        assert renderer.last_stages() == 2
        _band_check(oracle, p, W, H, whole, (0, 3000, 4096, 8188))
        banded = tuple(torch.full_like(t, -5) for t in whole)
        torch.cuda.synchronize()
        R = H // 8
        for rank in range(8):
            band = (rank + frame) % 8                                   # FrameExchange: rank r renders band (r + j) mod N
            sh = fr.Shard(band, 8, R)
            assert sh.rows(H) == R and int(sh.global_rows(H)[0]) == band * R
            renderer.render(st, W, H, rgba=banded[0][band * R:(band + 1) * R], nu=banded[1][band * R:(band + 1) * R],
                            iter=banded[2][band * R:(band + 1) * R], shard=sh)
        for x, y in zip(whole, banded):
            assert torch.equal(x, y), frame
        # the nu payload the ranks ship, recoloured at the destination, is the rendered colour plane bit for bit
        again = torch.empty_like(whole[0])
        renderer.colorize(st, banded[1], again)
        torch.cuda.synchronize()
        assert torch.equal(again, whole[0])
        del whole, banded, again


def test_strip_gather_pipeline_on_gpu(fr, renderer, oracle):
    """The N > 1 bench path's stream/event pipeline (compute stream -> comm stream, double buffering) on one
    GPU: world size 1 (no process group), strips of 8 rows, three frames submitted back to back."""
    import torch
    from fractalrenderer_amd.distributed import StripGather
    W, H = 160, 96
    dev = torch.device("cuda:0")
    sg = StripGather(W, H, 4, torch.float32, dev, rows_per_strip=8)
    states = [fr.FractalState(max_iterations=64 + 32 * k) for k in range(3)]

    def render_fn(shard, out, frame):
        renderer.render(states[frame], W, H, rgba=out, shard=shard, sync=False,
                        stream=torch.cuda.current_stream().cuda_stream)

    slots = [sg.submit(render_fn, k) for k in range(2)]
    sg.drain()
    for k, slot in enumerate(slots):
        ref = oracle.render(oracle.OracleParams(max_iterations=64 + 32 * k), W, H, planes=False).rgba
        assert np.abs(sg.frames[slot].cpu().numpy() - ref).max() <= RGB_TOL
    slot = sg.submit(render_fn, 2)          # reuses slot 0 after its gather finished
    sg.drain()
    ref = oracle.render(oracle.OracleParams(max_iterations=128), W, H, planes=False).rgba
    assert slot == 0 and np.abs(sg.frames[slot].cpu().numpy() - ref).max() <= RGB_TOL
    one = sg.render_frame(render_fn, 1)
    assert np.abs(one.cpu().numpy() - oracle.render(oracle.OracleParams(max_iterations=96), W, H, planes=False).rgba).max() <= RGB_TOL


def test_deep_zoom_larger_frame_and_planes(fr, renderer, oracle):
    """Deep_Zoom (shaders/test_deep_zoom.comp) at a size with ragged tiles, row-strip shard included."""
    p = oracle.OracleParams(fractal=5, precision=0, center_x=-0.743643887037151, center_y=0.13182590420533, zoom=3e-5,
                            max_iterations=1500, use_perturbation=1, palette_mode=0, color_scale=0.5)
    W, H = 203, 131
    ref = oracle.render(p, W, H)
    rgba, nu, it = gpu_render(fr, renderer, p, W, H)
    check_against(p, ref.iter, ref.nu, ref.rgba, rgba, nu, it)
    sh = fr.Shard(2, 3, 8)
    rows = sh.global_rows(H)
    rgba, nu, it = gpu_render(fr, renderer, p, W, H, shard=sh)
    check_against(p, ref.iter[rows], ref.nu[rows], ref.rgba[rows], rgba, nu, it)
    assert 0.05 < (ref.iter == 1500).mean() < 0.95          # the view shows both interior and exterior


def test_render_frame_png_end_to_end(fr, renderer, oracle, tmp_path):
    """The RenderFrameCallback body (src/vk_engine.cpp:1181-1418): render + post chain -> fp16 -> second ACES +
    gamma -> u8 -> flip -> PNG, against the oracle's restatement of the same chain."""
    from pngdec import read_png
    for kw, ft in ((dict(max_iterations=200), fr.FractalType.Mandelbrot),
                   (dict(max_iterations=300, center_x=0.0, julia_c_real=-0.8, julia_c_imag=0.156, palette_mode=6), fr.FractalType.JuliaSet)):
        W, H = 120, 72
        path = str(tmp_path / ("f%d.png" % int(ft)))
        assert renderer.render_frame(fr.FractalState(**kw), W, H, path, fractal_type=ft)
        px, _ = read_png(path)
        okw = {("max_iterations" if k == "max_iterations" else k): v for k, v in kw.items()}
        ref = oracle.render(oracle.OracleParams(fractal=int(ft), precision=0, post_chain=1, **okw), W, H, planes=False)
        want = oracle.export_rgb8(ref.rgba, through_half=True)
        # the export itself is byte-exact (test_export_rgb8); this tolerance is the RENDER's: its fp32 colour differs from
        # the oracle's in the last ulp or two (hardware exp2 / log2 in the palette warp and the post chain's gamma)
        d = np.abs(px.astype(np.int16) - want.astype(np.int16))
        assert px.shape == (H, W, 3) and d.max() <= 1 and (d > 0).mean() < 0.02
        # ... which the same chain applied to the library's own post-chained plane shows: identical bytes
        rgba_gpu = np.empty((H, W, 4), np.float32)
        renderer.render(fr.FractalState(**kw), W, H, fractal_type=ft, precision=fr.Precision.F32, rgba=rgba_gpu, post_chain=True)
        assert np.array_equal(px, oracle.export_rgb8(rgba_gpu, through_half=True))
    assert not renderer.render_frame(fr.FractalState(max_iterations=0), 8, 8, str(tmp_path / "bad.png"))


def test_export_rgb16(fr, renderer, oracle):
    p, W, H = CASES["c1_mandel_f64_default"]
    rgba, _, _ = gpu_render(fr, renderer, p, W, H)
    got = renderer.export_rgb16(rgba, W, H)
    want = (np.clip(rgba[::-1, :, :3], 0.0, 1.0) * np.float32(65535.0)).astype(np.uint16)     # src/vk_engine.cpp:2058-2069
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    half = renderer.export_rgb16(rgba, W, H, through_half=True)
    want_h = (np.clip(rgba[::-1, :, :3].astype(np.float16).astype(np.float32), 0.0, 1.0) * np.float32(65535.0)).astype(np.uint16)
    assert np.array_equal(half, want_h)


@pytest.mark.parametrize("name", sorted(n for n, (p, _, _) in CASES.items()
                                         if p.fractal <= 2 and p.aa <= 1 and not needs_effects(p)))
def test_colorize_reproduces_the_rendered_colour(fr, renderer, oracle, name):
    """fr_colorize_async: the colour plane recomputed from the nu plane is BIT-identical to the one the
    render kernels write (the multi-GPU exchange ships nu and recolours at the destination)."""
    import torch
    p, W, H = CASES[name]
    st = to_state(fr, p)
    ftype, prec = fr.FractalType(p.fractal), (fr.Precision.F64 if p.precision == 1 else fr.Precision.F32)
    supported = renderer.colorize_supported(st, ftype, prec)
    assert supported == ((p.bailout >= 2.5) if p.fractal == 0 else (p.bailout >= 1.25))
    dev = torch.device("cuda:0")
    for post in (False, True):
        rgba = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        nu = torch.empty((H, W), dtype=torch.float64 if p.precision == 1 else torch.float32, device=dev)
        renderer.render(st, W, H, fractal_type=ftype, precision=prec, post_chain=post, rgba=rgba, nu=nu)
        again = torch.full_like(rgba, -1.0)
        torch.cuda.synchronize()        # the fill ran on torch's stream, colorize runs on the context's own
        if not supported:
            with pytest.raises(fr.FractalRendererError) as e:
                renderer.colorize(st, nu, again, fractal_type=ftype, precision=prec, post_chain=post)
            assert e.value.status == fr._capi.FR_ERR_UNSUPPORTED
            continue
        renderer.colorize(st, nu, again, fractal_type=ftype, precision=prec, post_chain=post)
        torch.cuda.synchronize()
        assert torch.equal(again, rgba)
        if not post:
            ref = oracle.colorize(p, nu.cpu().numpy().astype(np.float64))
            assert np.abs(again.cpu().numpy() - ref).max() <= RGB_TOL


def test_colorize_rejects_effect_colourings(fr, renderer):
    st = fr.FractalState(orbit_trap_enabled=True)
    assert not renderer.colorize_supported(st)
    assert not renderer.colorize_supported(fr.FractalState(antialiasing_samples=2))
    assert not renderer.colorize_supported(fr.FractalState(), fr.FractalType.Deep_Zoom, fr.Precision.F32)
    assert not renderer.colorize_supported(fr.FractalState(interior_style=3), fr.FractalType.BurningShip)
    assert renderer.colorize_supported(fr.FractalState(interior_style=1))


def test_frame_exchange_single_rank_on_gpu(fr, renderer, oracle):
    """world 1 (no process group): FrameExchange degenerates to render -> assemble -> recolour on two
    streams; exercises the slot reuse events of the pipelined path."""
    import torch
    from fractalrenderer_amd.distributed import FrameExchange
    W, H = 160, 96
    dev = torch.device("cuda:0")
    states = [fr.FractalState(max_iterations=64 + 32 * k, palette_mode=k % 6) for k in range(5)]
    for payload in ("nu", "rgba"):
        fx = FrameExchange(W, H, payload=payload, device=dev, rows_per_strip=8)

        def render_fn(shard, out, frame, plane, lane=0):
            kw = {"nu": out} if plane == "nu" else {"rgba": out}
            renderer.render(states[frame], W, H, shard=shard, sync=False,
                            stream=torch.cuda.current_stream().cuda_stream, **kw)

        def colorize_fn(nu_frame, rgba_frame, frame):
            renderer.colorize(states[frame], nu_frame, rgba_frame, stream=torch.cuda.current_stream().cuda_stream)

        for k in range(5):
            slot = fx.submit_group(render_fn, k, 1, colorize_fn if payload == "nu" else None)
            fx.wait(slot)
            assert fx.frame_index[slot] == k
            ref = oracle.render(oracle.OracleParams(max_iterations=64 + 32 * k, palette_mode=k % 6), W, H)
            assert np.abs(fx.frame_rgba[slot].cpu().numpy() - ref.rgba).max() <= RGB_TOL
            if payload == "nu":
                assert np.abs(fx.frame_nu[slot].cpu().numpy() - ref.nu).max() <= NU_TOL_F64
        fx.drain()


def _fx_gpu_worker(rank, world, port, q, layout="strips"):
    import os
    import sys
    import torch
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import fractalrenderer_amd as fr
        from fractalrenderer_amd.distributed import FrameExchange
        W, H, nframes = 256, 192, 5
        dev = torch.device("cuda:0")
        r = fr.Renderer(0)
        r2 = fr.Renderer(0)                                          # second render context for lane 1
        states = [fr.FractalState(max_iterations=200 + 40 * k, zoom=3.0 - 0.2 * k) for k in range(nframes)]
        fx = FrameExchange(W, H, payload="nu", device=dev, render_lanes=2, layout=layout)   # gloo -> shares bounce through pinned host memory
        assert fx.stage and fx.bands == (layout == "bands")

        def render_fn(shard, out, frame, plane, lane=0):
            (r, r2)[lane].render(states[frame], W, H, shard=shard, sync=False, nu=out,
                                 stream=torch.cuda.current_stream().cuda_stream)

        def colorize_fn(nu_frame, rgba_frame, frame):
            r.colorize(states[frame], nu_frame, rgba_frame, stream=torch.cuda.current_stream().cuda_stream)

        fx.prime()
        ok, f = True, 0
        whole_rgba = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        whole_nu = torch.empty((H, W), dtype=torch.float64, device=dev)
        pending = []
        while f < nframes:
            count = min(world, nframes - f)
            slot = fx.submit_group(render_fn, f, count, colorize_fn)        # pipelined: no drain between groups
            pending.append((slot, f + rank if rank < count else -1))
            if len(pending) == 2:
                s0, fi = pending.pop(0)
                fx.wait(s0)
                if fi >= 0:
                    r.render(states[fi], W, H, rgba=whole_rgba, nu=whole_nu)
                    ok = ok and torch.equal(fx.frame_rgba[s0], whole_rgba) and torch.equal(fx.frame_nu[s0], whole_nu)
            f += count
        fx.drain()
        for s0, fi in pending:
            if fi >= 0:
                r.render(states[fi], W, H, rgba=whole_rgba, nu=whole_nu)
                ok = ok and torch.equal(fx.frame_rgba[s0], whole_rgba) and torch.equal(fx.frame_nu[s0], whole_nu)
        r2.close()
        r.close()
        q.put((rank, ok))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("layout", ["strips", "bands"])
def test_frame_exchange_two_ranks_sharing_the_card(fr, layout):
    """Rehearsal of the N > 1 GPU path on ONE card: 2 processes, gloo rendezvous, shares bounced through
    pinned host memory (RCCL refuses two ranks on one device).  Every frame delivered to rank
    (frame mod 2) must equal, bitwise, a whole-frame render of the same state.  Both layouts: interleaved row strips,
    and contiguous bands that rotate over the frames of a group and are received in place."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_fx_gpu_worker, args=(r, 2, port, q, layout)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    for _ in range(2):
        rank, ok = q.get(timeout=5)
        assert ok, rank


def test_library_first_then_torch_share_one_hip_runtime():
    """Import order must not matter: the library loaded (and a context created) BEFORE torch is imported
    must leave torch able to see the GPU, and torch memory usable by the library."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import fractalrenderer_amd as fr\n"
            "assert 'torch' not in sys.modules\n"
            "r = fr.Renderer(0)\n"
            "import torch\n"
            "nu = torch.zeros((64, 64), dtype=torch.float64, device='cuda:0')\n"
            "r.render(fr.FractalState(), 64, 64, nu=nu)\n"
            "assert float(nu.max()) == 256.0 and float(nu.min()) > 0.0\n"
            "r.close(); print('ok')\n") % root
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


@pytest.mark.parametrize("W,H", [(1, 1), (8, 8), (64, 8), (100, 37), (520, 16)])
def test_limited_probing_on_small_grids(fr, renderer, oracle, W, H):
    """Waves that stop after their home shard (probes=1) must still cover every shard, whatever the grid
    size: grids smaller than the shard count fall back to full probing, larger ones take the home shard
    from the workgroup index."""
    p = oracle.OracleParams(max_iterations=200, center_x=-0.75, zoom=2.0)
    ref = oracle.render(p, W, H)
    try:
        for probes, wg in ((1, 0), (2, 0), (1, 1)):
            renderer.set_option("probes", probes)
            renderer.set_tuning(wg, 0, 0)
            rgba, nu, it = gpu_render(fr, renderer, p, W, H)
            check_against(p, ref.iter, ref.nu, ref.rgba, rgba, nu, it)
    finally:
        renderer.set_option("probes", 0)
        renderer.set_tuning()


def _anim_export_worker(rank, world, port, out_dir, q):
    import os
    import sys
    import torch
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import fractalrenderer_amd as fr
        from fractalrenderer_amd.distributed import export_animation
        anim = fr.AnimationSystem()
        assert anim.load_from_file(os.path.join(root, "tests", "golden", "reference_sample.franim"))
        rs = [fr.Renderer(0), fr.Renderer(0)]
        frames = [0, 480, 1111, 1700, 2399]                # 5 frames: two full groups of 2 + a partial one
        written = export_animation(anim, rs, out_dir, precision=fr.Precision.F32, width=192, height=128,
                                   frames=frames, device=torch.device("cuda:0"))
        for r in rs:
            r.close()
        q.put((rank, sorted(written)))
    finally:
        dist.destroy_process_group()


def test_distributed_animation_export_matches_single_gpu_pngs(fr, renderer, tmp_path):
    """The C5 pipeline end to end on one card (2 ranks, gloo, strips through pinned host memory): .franim ->
    interpolate -> row-strip renders of the nu plane -> exchange -> recolour with the post chain -> 8-bit export
    -> PNG.  Every file must be byte-identical to the one the single-GPU RenderFrameCallback body writes."""
    import os
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out_dir = str(tmp_path / "dist"); os.makedirs(out_dir)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_anim_export_worker, args=(r, 2, port, out_dir, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    got = {}
    for _ in range(2):
        rank, written = q.get(timeout=5)
        got[rank] = written
    frames = [0, 480, 1111, 1700, 2399]
    assert [os.path.basename(x) for x in got[0]] == ["frame_%06d.png" % f for f in (0, 1111, 2399)]   # positions 0, 2, 4
    assert [os.path.basename(x) for x in got[1]] == ["frame_%06d.png" % f for f in (480, 1700)]
    anim = fr.AnimationSystem()
    assert anim.load_from_file(os.path.join(os.path.dirname(__file__), "golden", "reference_sample.franim"))
    for f in frames:
        ref_path = str(tmp_path / ("ref_%06d.png" % f))
        assert renderer.render_frame(anim.interpolate(anim.frame_time(f)), 192, 128, ref_path)
        assert open(ref_path, "rb").read() == open(os.path.join(out_dir, "frame_%06d.png" % f), "rb").read(), f


@pytest.mark.parametrize("n,slots", [(1, 2), (3, 4)])
def test_node_render_animation_matches_single_gpu_pngs(fr, renderer, tmp_path, n, slots):
    """fr_node_render_animation: AnimationRenderer::start_render over the parts of a node, from C -- the reference's own
    .franim, every 300th frame of its 2400, frames in flight, roots rotating, the 8-bit export where the frame was assembled,
    a writer thread for the PNGs.  Every file byte-identical to the single-GPU RenderFrameCallback body's
    (fr_render_frame_png); the callback sees every frame in order and can cancel; fewer than 2 keyframes are refused."""
    anim = fr.AnimationSystem()
    assert anim.load_from_file(os.path.join(os.path.dirname(__file__), "golden", "reference_sample.franim"))
    out_dir = str(tmp_path / "nested" / "out")                      # created by the call (create_directories)
    seen = []
    with fr.Node([0] * n) as node:
        node.set_option("slots", slots)
        wrote = node.render_animation(anim, out_dir, width=200, height=136, frame_step=300, precision=fr.Precision.F32,
                                      on_frame_complete=lambda f, t: seen.append((f, t)) and False)
        frames = list(range(0, 2400, 300))
        assert wrote == len(frames) and seen == [(f, 2400) for f in frames]
        assert sorted(os.listdir(out_dir)) == ["frame_%06d.png" % f for f in frames]
        for f in frames:
            ref_path = str(tmp_path / ("ref_%06d.png" % f))
            assert renderer.render_frame(anim.interpolate(anim.frame_time(f)), 200, 136, ref_path)
            assert open(ref_path, "rb").read() == open(os.path.join(out_dir, "frame_%06d.png" % f), "rb").read(), f
        # a window of the sequence, fp64, with an iteration override; cancelled by the callback after its third frame
        out2 = str(tmp_path / "win")
        count = []
        wrote = node.render_animation(anim, out2, width=96, height=64, first_frame=1000, frame_count=40, frame_step=2,
                                      precision=fr.Precision.F64, max_iterations=700,
                                      on_frame_complete=lambda f, t: count.append(f) or len(count) >= 3)
        assert 3 <= wrote < 20 and count[:3] == [1000, 1002, 1004] and node.in_flight() == 0
        st = anim.interpolate(anim.frame_time(1002))
        st.max_iterations = 700
        ref_path = str(tmp_path / "ref_win.png")
        assert renderer.render_frame(st, 96, 64, ref_path, precision=fr.Precision.F64)
        assert open(ref_path, "rb").read() == open(os.path.join(out2, "frame_001002.png"), "rb").read()
        # the perturbation shader's frames (no post chain in the shader: fr_render_frame_png's rule), two frames
        out3 = str(tmp_path / "dz")
        assert node.render_animation(anim, out3, width=80, height=64, first_frame=2390, frame_count=2, fractal_type=fr.FractalType.Deep_Zoom) == 2
        ref_path = str(tmp_path / "ref_dz.png")
        assert renderer.render_frame(anim.interpolate(anim.frame_time(2391)), 80, 64, ref_path, fractal_type=fr.FractalType.Deep_Zoom)
        assert open(ref_path, "rb").read() == open(os.path.join(out3, "frame_002391.png"), "rb").read()
        one = fr.AnimationSystem()
        one.add_keyframe(0.0, fr.FractalState())
        with pytest.raises(fr.FractalRendererError) as e:
            node.render_animation(one, str(tmp_path / "none"))
        assert "at least 2 keyframes" in str(e.value) and not os.path.exists(str(tmp_path / "none"))


def test_node_render_animation_into_a_pipe(fr, renderer, tmp_path):
    """fr_anim_render_options.raw_fd: the frames of an animation as packed RGB24 into a file descriptor -- what an encoder
    reads from its stdin (`ffmpeg -f rawvideo -pix_fmt rgb24`, src/video_encoder.cpp:195-224) -- instead of PNG files: no
    deflate between the GPUs and the encoder.  Through an OS pipe with a reader thread; every frame's bytes are the pixels
    the PNG path writes (fr_export_rgb8 of the post-chained frame, fp16 rounding included), in frame order; no folder is
    created or needed."""
    import threading
    import torch
    anim = fr.AnimationSystem()
    assert anim.load_from_file(os.path.join(os.path.dirname(__file__), "golden", "reference_sample.franim"))
    W, H = 264, 152
    frames = list(range(100, 2400, 400))
    rd, wr = os.pipe()
    got = bytearray()

    def reader():
        with os.fdopen(rd, "rb") as f:
            while True:
                b = f.read(1 << 16)
                if not b:
                    break
                got.extend(b)
    th = threading.Thread(target=reader)
    th.start()
    seen = []
    try:
        with fr.Node([0, 0, 0]) as node:
            wrote = node.render_animation(anim, None, width=W, height=H, first_frame=100, frame_step=400, precision=fr.Precision.F64,
                                          raw_fd=wr, on_frame_complete=lambda f, t: seen.append(f) and False)
    finally:
        os.close(wr)
        th.join(60)
    assert wrote == len(frames) and seen == frames
    assert len(got) == len(frames) * W * H * 3
    rgba = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    for k, f in enumerate(frames):
        renderer.render(anim.interpolate(anim.frame_time(f)), W, H, precision=fr.Precision.F64, post_chain=True, rgba=rgba)
        want = renderer.export_rgb8(rgba, W, H, through_half=True).cpu().numpy().tobytes()
        assert bytes(got[k * W * H * 3:(k + 1) * W * H * 3]) == want, f
    assert not os.path.exists(str(tmp_path / "anything"))
    with fr.Node([0]) as node:                                   # neither a folder nor a descriptor: refused
        with pytest.raises(fr.FractalRendererError):
            node.render_animation(anim, None, width=W, height=H)
        # an encoder that has gone away: the export stops with an I/O error (no hang, nothing left in flight), and the node
        # renders on afterwards
        rd, wr = os.pipe()
        os.close(rd)
        try:
            with pytest.raises(fr.FractalRendererError) as e:
                node.render_animation(anim, None, width=W, height=H, first_frame=100, frame_step=400, precision=fr.Precision.F64, raw_fd=wr)
            assert e.value.status == fr._capi.FR_ERR_IO and node.in_flight() == 0
        finally:
            os.close(wr)
        out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
        node.render(anim.interpolate(anim.frame_time(100)), W, H, precision=fr.Precision.F64, post_chain=True, rgba=out)
        renderer.render(anim.interpolate(anim.frame_time(100)), W, H, precision=fr.Precision.F64, post_chain=True, rgba=rgba)
        assert torch.equal(out, rgba)


def test_randomised_views_match_the_oracle(fr, renderer, oracle):
    """Seeded sweep over the parameter space (fractal, precision, view, iteration budget, bailout, palette,
    frame shape, row-strip shard): escape indices bit-exact, nu and colour within the stated bars.  Views are
    drawn around points of the sets' boundaries so that frames mix interior, slow and fast escapes."""
    rng = np.random.default_rng(20261004)
    anchors = {0: [(-0.743643887037151, 0.13182590420533), (-0.1011, 0.9563), (-1.25066, 0.02012), (0.275, 0.0),
                   (-0.5, 0.0), (-1.7497, 0.00001)],
               1: [(0.0, 0.0), (0.3, 0.2), (-0.6, 0.1)],
               2: [(-1.755, -0.03), (-0.5, -0.5), (-1.62, -0.002)]}
    for trial in range(48):
        fractal = int(rng.integers(0, 3))
        prec = int(rng.integers(0, 2))
        ax, ay = anchors[fractal][int(rng.integers(0, len(anchors[fractal])))]
        zoom = float(10.0 ** rng.uniform(-4.0 if prec == 1 else -2.0, 0.6))
        W, H = int(rng.integers(9, 180)), int(rng.integers(5, 120))
        kw = dict(fractal=fractal, precision=prec, center_x=ax + zoom * float(rng.uniform(-0.2, 0.2)),
                  center_y=ay + zoom * float(rng.uniform(-0.2, 0.2)), zoom=zoom,
                  max_iterations=int(rng.choice([1, 7, 33, 64, 127, 128, 129, 300, 777, 1500, 3000])),
                  bailout=float(rng.choice([1.5, 2.0, 2.5, 4.0, 4.0, 4.0, 16.0, 1000.0])),
                  palette_mode=int(rng.integers(0, 6 if fractal == 0 else 10)),
                  color_offset=float(np.float32(rng.uniform(0, 1))), color_scale=float(np.float32(rng.uniform(0.5, 6))),
                  interior_style=int(rng.choice([0, 0, 1])), post_chain=int(rng.integers(0, 2)))
        if fractal == 1:
            kw.update(julia_c_real=float(rng.uniform(-0.9, 0.4)), julia_c_imag=float(rng.uniform(-0.7, 0.7)))
        p = oracle.OracleParams(**kw)
        ref = oracle.render(p, W, H)
        shard = None
        if trial % 3 == 1:
            nparts = int(rng.integers(2, 6))
            shard = fr.Shard(int(rng.integers(0, nparts)), nparts, int(rng.integers(1, 9)))
        rgba, nu, it = gpu_render(fr, renderer, p, W, H, shard=shard)
        rows = shard.global_rows(H) if shard else slice(None)
        try:
            check_against(p, ref.iter[rows], ref.nu[rows], ref.rgba[rows], rgba, nu, it)
        except AssertionError as e:
            raise AssertionError("trial %d %r %dx%d shard %r: %s" % (trial, kw, W, H, shard, e))


def test_contexts_release_their_device_memory(fr):
    """Create / render / destroy cycles must give the device memory back (survivor streams, control
    blocks, orbit and frame buffers are all context-owned)."""
    import torch
    torch.cuda.synchronize()
    st = fr.FractalState(max_iterations=600)
    out = torch.empty((512, 512, 4), dtype=torch.float32, device="cuda:0")

    def cycle():
        r = fr.Renderer(0)
        r.render(st, 512, 512, rgba=out)
        r.render(fr.FractalState(max_iterations=500, zoom=1e-4, use_perturbation=True), 256, 256,
                 fractal_type=fr.FractalType.Deep_Zoom, precision=fr.Precision.F32, rgba=out[:128].reshape(256, 256, 4)[:256])
        r.close()

    cycle()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(20):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (8 << 20), "leaked %d bytes over 20 create/destroy cycles" % (free0 - free1)


def test_plain_c_client_renders_through_the_abi(fr, tmp_path):
    """tests/c_client/client.c (C11, public header only, no Python / torch in the process): render to host
    buffers, analytic known answers, conjugate symmetry, shard == rows of the frame, export, PNG, error codes."""
    import subprocess
    from test_host import build_c_client
    exe = build_c_client(tmp_path)
    out = subprocess.run([exe, "gpu", str(tmp_path / "g.png")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "gpu ok", out.stderr


def test_automatic_cycle_closing_stops_looking_where_nothing_closes(fr):
    """"periodicity" = 0 (automatic): a context whose lane pools looked and closed nothing -- a Julia dust -- renders its
    next frames of the same kind with the plain lane pool and looks again every 16th; one whose pools close cycles keeps
    looking; an explicit setting is obeyed; and the planes never depend on any of it."""
    import torch
    W, H = 320, 200
    dust = dict(state=fr.FractalState(max_iterations=2048, center_x=0.0, julia_c_real=-0.8, julia_c_imag=0.156),
                fractal_type=fr.FractalType.JuliaSet, precision=fr.Precision.F32)
    filled = dict(state=fr.FractalState(max_iterations=1024), fractal_type=fr.FractalType.Mandelbrot, precision=fr.Precision.F64)
    with fr.Renderer(0) as r:
        r.set_option("staging", 3)                 # (a frame this small takes one pass by itself up to max_iter 1536)
        for case, expect_looks in ((dust, "few"), (filled, "all")):
            nu_dt = torch.float64 if case["precision"] == fr.Precision.F64 else torch.float32
            want = torch.empty((H, W), dtype=nu_dt, device="cuda")
            r.set_option("periodicity", -1)
            r.render(case["state"], W, H, fractal_type=case["fractal_type"], precision=case["precision"], nu=want)
            assert r.last_stages() == 2 and r.last_pool_closing() == 0
            r.set_option("periodicity", 1)
            r.render(case["state"], W, H, fractal_type=case["fractal_type"], precision=case["precision"], nu=want.clone())
            assert r.last_pool_closing() == 1
            r.set_option("periodicity", 0)
            looks = []
            for _ in range(40):
                got = torch.zeros_like(want)
                r.render(case["state"], W, H, fractal_type=case["fractal_type"], precision=case["precision"], nu=got)
                assert torch.equal(got, want)
                looks.append(r.last_pool_closing())
            if expect_looks == "all":
                assert all(v == 1 for v in looks), looks
            else:
                assert looks[0] == 1 and 2 <= sum(looks) <= 12, looks          # the first frames, then one look in 16
                assert sum(looks[:4]) >= 2 and 1 in looks[16:], looks
        # a one-pass frame has no lane pool
        r.set_option("staging", 0)
        r.render(fr.FractalState(max_iterations=100), W, H, nu=torch.empty((H, W), dtype=torch.float64, device="cuda"))
        assert r.last_pool_closing() == -1
        r.set_option("staging", 3)
        # a sequence that leaves the dust for a filled Julia set (same fractal, size, max_iter: only the view's constant
        # changes) starts looking again at once, and keeps looking there
        r.set_option("periodicity", 0)
        looks = []
        for _ in range(20):
            r.render(dust["state"], W, H, fractal_type=dust["fractal_type"], precision=dust["precision"], nu=torch.empty((H, W), dtype=torch.float32, device="cuda"))
            looks.append(r.last_pool_closing())
        assert looks[-1] == 0 or sum(looks[-8:]) <= 2, looks                                 # not looking (any more)
        rabbit = fr.FractalState(max_iterations=2048, center_x=0.0, julia_c_real=-0.123, julia_c_imag=0.745)
        looks = []
        for _ in range(6):
            r.render(rabbit, W, H, fractal_type=fr.FractalType.JuliaSet, precision=fr.Precision.F32, nu=torch.empty((H, W), dtype=torch.float32, device="cuda"))
            looks.append(r.last_pool_closing())
        assert looks == [1] * 6, looks


def test_plain_c_node_client_on_one_card(fr, tmp_path):
    """tests/c_client/node_client.c: the C-ABI multi-GPU entry points from plain C.  `lanes`: n = 2, 4, 8 parts that are all
    device 0 -- strips and bands, every root, in-place stores into one set of whole-frame planes -- bitwise against
    fr_render; `rccl`: plugin load, communicator life cycle and a grouped ncclSend / ncclRecv pair on this card."""
    import subprocess
    from test_host import build_c_client
    exe = build_c_client(tmp_path, "node_client.c")
    out = subprocess.run([exe, "lanes"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip() == "lanes ok", out.stderr + out.stdout
    out = subprocess.run([exe, "rccl"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("rccl ok"), out.stderr + out.stdout


def test_plain_c_node_client_frames_in_flight(fr, tmp_path):
    """`seq`: a 16-frame sequence on devices = {0} and {0,0,0,0} with 1..8 frame slots and 1..4 render lanes, rotating roots,
    tickets waited for in a scrambled order, every frame bitwise against fr_render; a node destroyed with frames in flight."""
    import subprocess
    from test_host import build_c_client
    exe = build_c_client(tmp_path, "node_client.c")
    out = subprocess.run([exe, "seq"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.strip() == "seq ok", out.stderr + out.stdout


def test_plain_c_node_client_animation(fr, tmp_path):
    """`anim`: fr_node_render_animation from plain C -- keyframes added through the ABI, every 10th frame over two parts,
    the callback in order, every PNG byte for byte fr_render_frame_png's."""
    import subprocess
    from test_host import build_c_client
    exe = build_c_client(tmp_path, "node_client.c")
    out = subprocess.run([exe, "anim", str(tmp_path / "frames" / "a")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "anim ok", out.stderr + out.stdout


def test_plain_c_node_client_gather_failure_paths(fr, tmp_path):
    """`failsafe`: a part that fails before its render (reported under its frame's ticket, the node stays usable); a whole
    frame through the RCCL calls of a one-rank communicator ("rccl_loopback": packed staging, grouped send / recv on the comm
    stream, in-place receives, the smooth-count payload recoloured), two frames in flight; a part that fails between the
    two-phase barrier and its sends: the communicators are aborted, the wait returns the error within its bound and the
    node carries on with the in-place gather."""
    import subprocess
    from test_host import build_c_client
    exe = build_c_client(tmp_path, "node_client.c")
    out = subprocess.run([exe, "failsafe"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("failsafe ok"), out.stderr + out.stdout      # (RCCL prints a banner)


def test_rccl_plugin_next_to_torch(fr):
    """The RCCL leg of fr_node inside a process that holds PyTorch's bundled HIP runtime and RCCL (this one: torch is
    imported and its CUDA context is up): the plugin loads, a one-rank communicator carries a grouped send / recv pair, and
    a whole frame goes through the loopback gather, bitwise equal to fr_render -- with ONE libamdhip64 mapped."""
    import torch
    assert torch.cuda.is_available()
    torch.zeros(4, device="cuda").sum().item()                      # torch's runtime is initialised before the plugin loads
    assert fr.rccl_selftest(0, 1 << 20) > 0
    W, H = 264, 136
    st = fr.FractalState(max_iterations=1024)
    want = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    with fr.Renderer(0) as r:
        r.render(st, W, H, rgba=want)
    with fr.Node([0]) as node:
        node.set_tuning("rccl_loopback", 1)
        node.set_option("gather", fr._capi.FR_GATHER_RCCL)
        got = torch.zeros_like(want)
        torch.cuda.synchronize()                                    # the fill runs on torch's stream
        node.render(st, W, H, rgba=got)
        assert node.last_gather() == fr._capi.FR_GATHER_RCCL and node.rccl_usable()
        assert torch.equal(got, want)
    maps = fr.mapped_runtimes()
    print("mapped runtimes:", maps)
    hips = {os.path.realpath(m) for m in maps if "libamdhip64" in m}
    assert len(hips) == 1, maps
    assert any("librccl" in m for m in maps), maps


def test_staged_ssaa_is_bit_identical_to_the_sample_loop(fr, renderer):
    """SSAA two ways: the sample loop of the general tile kernel ("ssaa" = 1: a pixel's aa x aa samples one after the other in
    lockstep) and the staged form ("ssaa" = 2: the sample grid rendered as a frame of its own through the lean tile pass and the
    lane pool -- its coordinate tables hold the shaders' sample positions --, then averaged in the shader's order).  Every
    plane must be bit-identical: Mandelbrot / Julia / Burning Ship (sy-outer and sx-outer sample orders), fp64 / fp32, aa 2
    and 3, post chain, ragged sizes, row strips (packed and whole-frame planes) and the automatic choice."""
    import torch
    cases = [(fr.FractalType.Mandelbrot, fr.Precision.F64, dict(max_iterations=1024)),
             (fr.FractalType.Mandelbrot, fr.Precision.F32, dict(max_iterations=900, center_x=-0.743643887037151, center_y=0.13182590420533, zoom=0.02)),
             (fr.FractalType.JuliaSet, fr.Precision.F32, dict(max_iterations=800, center_x=0.0, julia_c_real=-0.8, julia_c_imag=0.156)),
             (fr.FractalType.JuliaSet, fr.Precision.F64, dict(max_iterations=300, center_x=0.0, julia_c_real=-0.123, julia_c_imag=0.745)),
             (fr.FractalType.BurningShip, fr.Precision.F64, dict(max_iterations=600, center_x=-1.755, center_y=-0.03, zoom=0.1))]
    W, H = 203, 118
    try:
        for ft, prec, kw in cases:
            nu_dt = torch.float64 if prec == fr.Precision.F64 else torch.float32
            for aa, post in ((2, False), (3, True)):
                st = fr.FractalState(antialiasing_samples=aa, **kw)

                def run(mode, shard=None, rows=H):
                    renderer.set_option("ssaa", mode)
                    out = (torch.full((rows, W, 4), -1.0, dtype=torch.float32, device="cuda"), torch.full((rows, W), -1.0, dtype=nu_dt, device="cuda"),
                           torch.full((rows, W), -1, dtype=torch.int32, device="cuda"))
                    torch.cuda.synchronize()
                    renderer.render(st, W, H, fractal_type=ft, precision=prec, post_chain=post, rgba=out[0], nu=out[1], iter=out[2], shard=shard)
                    return out

                want = run(1)
                assert renderer.last_stages() == 1                              # the sample loop is one pass
                got = run(2)
                for a, b in zip(want, got):
                    assert torch.equal(a, b), (ft, prec, aa)
                auto = run(0)
                for a, b in zip(want, auto):
                    assert torch.equal(a, b), (ft, prec, aa, "auto")
                # a sample grid larger than the band size goes through the scratch in bands of whole sub-tile rows (print-export
                # sizes: above 2^29 samples; here the band size is set small: 118 rows in bands of 8, 16, 40, 112 rows)
                for band in (W * aa * aa * 8, W * aa * aa * 23, W * aa * aa * 40, W * aa * aa * 117):
                    renderer.set_option("ssaa_band_samples", band)
                    banded = run(0)
                    renderer.set_option("ssaa_band_samples", 0)
                    for a, b in zip(want, banded):
                        assert torch.equal(a, b), (ft, prec, aa, "bands", band)
                for part in range(3):                                           # strips of 8 rows: whole sub-tile rows in sample space
                    sh = fr.Shard(part, 3, 8)
                    rows = sh.rows(H)
                    w2, g2 = run(1, sh, rows), run(2, sh, rows)
                    for a, b in zip(w2, g2):
                        assert torch.equal(a, b), (ft, prec, aa, part)
                    idx = torch.from_numpy(sh.global_rows(H)).to("cuda")
                    assert torch.equal(g2[0], want[0][idx]) and torch.equal(g2[2], want[2][idx])
        # through fr_node: whole-frame planes (FR_LAYOUT_FRAME), two parts
        st = fr.FractalState(antialiasing_samples=2, max_iterations=1024)
        renderer.set_option("ssaa", 1)
        want = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        renderer.render(st, W, H, rgba=want)
        with fr.Node([0, 0]) as node:
            node.set_tuning("ssaa", 2)
            got = torch.zeros_like(want)
            torch.cuda.synchronize()
            node.render(st, W, H, rgba=got)
            assert torch.equal(got, want)
    finally:
        renderer.set_option("ssaa", 0)
        renderer.set_option("ssaa_band_samples", 0)


def test_bench_node_host_and_default_lines(fr):
    """bench.py keeps its contract on the C-ABI host: `--host node` (ONE process, fr_node: every gather x mode pair the box
    allows, here with two parts on this card and the one-rank RCCL loopback with one) prints ONE JSON line with the
    contract's keys, a `node` object whose runs are all verified against fr_render -- and the default command's line still
    carries roofline + roofline_valu (cpu_baseline switched off here for time)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def line(*flags):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "c1", "--steps", "4", "--warmup", "1", *flags],
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out.stdout
        return json.loads(lines[0])

    for parts in (1, 2):
        d = line("--host", "node", "--gpus", "1", "--node-parts", str(parts))
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                  "dtype", "data", "config", "roofline"):
            assert k in d, k
        assert d["host"] == "node" and d["value"] > 0 and d["exchange_verified"] is True
        runs = d["node"]["runs"]
        assert all("error" not in r and r["exchange_verified"] for r in runs), runs
        assert {r["mode"] for r in runs} == {"sequence", "frame"}
        assert any(r["gather"] == "rccl" for r in runs) == (parts == 1)          # the loopback needs a node of one part
    d = line("--no-cpu-baseline")
    assert d["n_gpus"] == 1 and "roofline" in d and "roofline_valu" in d and d["roofline"]["kernel_ms"] > 0


@pytest.mark.parametrize("workload", ["c1", "c2"])
def test_bench_dump_outputs_is_the_rendered_frame(fr, tmp_path, workload):
    """bench.py --dump-outputs DIR: after K timed steps DIR/rgba.npy holds the colour plane of the last step -- the whole
    plane for C1 (4 MB), for C2 (256 MB) the seeded 2^20-pixel sample beside its indices -- bitwise equal to a direct
    render of the same frame; the line reports K steps and their ms_per_step."""
    import json
    import subprocess
    import sys
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import bench
    out_dir = str(tmp_path / "dump")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", workload, "--steps", "3", "--warmup", "1",
                          "--no-cpu-baseline", "--no-periodicity", "--dump-outputs", out_dir],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["dump_outputs"]["dir"] == out_dir
    w = bench.WORKLOADS[workload]
    W, H = w["W"], w["H"]
    want = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    with fr.Renderer(0) as r:
        r.render(fr.FractalState(**w["state"]), W, H, fractal_type=fr.FractalType[w["fractal"]],
                 precision=fr.Precision[w["precision"]], rgba=want)
    want = want.cpu().numpy()
    got = np.load(os.path.join(out_dir, "rgba.npy"))
    assert got.dtype == np.float32
    if workload == "c1":
        assert not d["dump_outputs"]["sampled"] and sorted(os.listdir(out_dir)) == ["rgba.npy"]
        assert np.array_equal(got, want)
    else:
        idx = np.load(os.path.join(out_dir, "pixel_index.npy"))
        assert d["dump_outputs"]["sampled"] and idx.dtype == np.float64 and idx.shape == (1 << 20,)
        assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir)) <= 64 << 20
        assert np.array_equal(got, want.reshape(H * W, 4)[idx.astype(np.int64)])


@pytest.mark.parametrize("n,slots,lanes", [(1, 2, 2), (4, 3, 2), (8, 8, 4)])
def test_node_frames_in_flight_device_planes(fr, renderer, n, slots, lanes):
    """fr_node_submit / fr_node_wait_frame with device planes: 12 different frames, up to `slots` in flight on `lanes` render
    contexts per part, each into its own planes on the card, waited for newest first; bitwise against fr_render."""
    import torch
    W, H = 328, 203
    frames = []
    for f in range(12):
        if f % 3 == 2:
            frames.append((fr.FractalState(max_iterations=900, center_x=0.0, zoom=3.0 - 0.1 * f, julia_c_real=-0.8, julia_c_imag=0.156),
                           fr.FractalType.JuliaSet, fr.Precision.F32))
        else:
            frames.append((fr.FractalState(max_iterations=1024 if f % 3 else 200, zoom=3.0 - 0.15 * f), fr.FractalType.Mandelbrot, fr.Precision.F64))
    want = []
    for st, ft, prec in frames:
        nu_dt = torch.float64 if prec == fr.Precision.F64 else torch.float32
        w = (torch.empty((H, W, 4), dtype=torch.float32, device="cuda"), torch.empty((H, W), dtype=nu_dt, device="cuda"))
        renderer.render(st, W, H, fractal_type=ft, precision=prec, rgba=w[0], nu=w[1])
        want.append(w)
    with fr.Node([0] * n) as node:
        node.set_option("slots", slots); node.set_option("lanes", lanes)
        got = [tuple(torch.zeros_like(t) for t in w) for w in want]
        torch.cuda.synchronize()                                    # the fills run on torch's stream
        tickets = [node.submit(st, W, H, root=f % n, fractal_type=ft, precision=prec, rgba=got[f][0], nu=got[f][1])
                   for f, (st, ft, prec) in enumerate(frames)]
        assert tickets == list(range(tickets[0], tickets[0] + 12)) and 1 <= node.in_flight() <= slots
        for f in reversed(range(12)):
            node.wait_frame(tickets[f])
            assert torch.equal(got[f][0], want[f][0]) and torch.equal(got[f][1], want[f][1]), f
        assert node.in_flight() == 0
        with pytest.raises(fr.FractalRendererError):
            node.wait_frame(tickets[-1] + 1)


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_node_render_equals_fr_render(fr, renderer, n):
    """fr_node_render with n parts on this one card against fr_render, bitwise: device and host planes, strips / bands /
    explicit strip heights (whole sub-tile rows: the lean tile kernel; 5 rows: the general one), every kind of kernel
    behind the parts (two-pass fp64, Julia fp32, SSAA, effects, Deep_Zoom), rotating roots, async + wait."""
    import torch
    W, H = 328, 203
    cases = [(dict(max_iterations=1024), fr.FractalType.Mandelbrot, fr.Precision.F64),
             (dict(max_iterations=800, center_x=0.0, julia_c_real=-0.8, julia_c_imag=0.156), fr.FractalType.JuliaSet, fr.Precision.F32),
             (dict(max_iterations=120, antialiasing_samples=2), fr.FractalType.Mandelbrot, fr.Precision.F64),
             (dict(max_iterations=150, orbit_trap_enabled=True), fr.FractalType.Mandelbrot, fr.Precision.F32),
             (dict(max_iterations=300, center_x=-0.743643887037151, center_y=0.13182590420533, zoom=1e-3, use_perturbation=True),
              fr.FractalType.Deep_Zoom, fr.Precision.F32)]
    with fr.Node([0] * n) as node:
        for kw, ft, prec in cases:
            st = fr.FractalState(**kw)
            nu_dt = torch.float64 if prec == fr.Precision.F64 else torch.float32
            want = (torch.empty((H, W, 4), dtype=torch.float32, device="cuda"), torch.empty((H, W), dtype=nu_dt, device="cuda"),
                    torch.empty((H, W), dtype=torch.int32, device="cuda"))
            renderer.render(st, W, H, fractal_type=ft, precision=prec, rgba=want[0], nu=want[1], iter=want[2])
            for opts in (dict(), dict(layout=1), dict(rows_per_strip=8), dict(rows_per_strip=5), dict(rows_per_strip=64)):
                for k in ("layout", "rows_per_strip"):
                    node.set_option(k, opts.get(k, 0))
                root = (len(opts) + n - 1) % n
                got = tuple(torch.zeros_like(t) for t in want)
                node.render(st, W, H, root=root, fractal_type=ft, precision=prec, rgba=got[0], nu=got[1], iter=got[2])
                assert node.last_gather() == fr._capi.FR_GATHER_PEER
                for a, b in zip(want, got):
                    assert torch.equal(a, b), (kw, opts, n)
            node.set_option("layout", 0); node.set_option("rows_per_strip", 0)
            # host planes (staged through a frame on the root), colour only; async
            rgba_h = np.zeros((H, W, 4), np.float32)
            node.render(st, W, H, root=n - 1, fractal_type=ft, precision=prec, rgba=rgba_h, sync=False)
            node.wait()
            assert np.array_equal(rgba_h, want[0].cpu().numpy()), kw
        with pytest.raises(fr.FractalRendererError):
            node.render(fr.FractalState(), W, H, root=n, rgba=rgba_h)
        if n > 1:
            node.set_option("gather", fr._capi.FR_GATHER_RCCL)
            with pytest.raises(fr.FractalRendererError) as e:
                node.render(fr.FractalState(), W, H, rgba=rgba_h)
            assert e.value.status == fr._capi.FR_ERR_UNSUPPORTED


def test_whole_frame_layout_of_a_shard(fr, renderer):
    """FR_LAYOUT_FRAME: a part stores its rows in place into whole-frame planes; rows of other parts stay untouched."""
    import torch
    W, H = 200, 120
    st = fr.FractalState(max_iterations=900)
    want = torch.empty((H, W), dtype=torch.float64, device="cuda")
    renderer.render(st, W, H, nu=want)
    for nparts, R in ((3, 8), (2, 5), (4, 16)):
        frame = torch.full((H, W), -1.0, dtype=torch.float64, device="cuda")
        for part in (0, nparts - 1):
            sh = fr.Shard(part, nparts, R)
            p = st.to_params(fr.FractalType.Mandelbrot, fr.Precision.F64)
            out = fr._capi.fr_output(None, frame.data_ptr(), None, fr._capi.FR_MEM_DEVICE, fr._capi.FR_LAYOUT_FRAME)
            shc = sh.to_c()
            fr._capi.check(fr.lib().fr_render_shard(renderer._ctx, C.byref(p), W, H, C.byref(shc), C.byref(out)))
            rows = torch.from_numpy(sh.global_rows(H)).cuda()
            assert torch.equal(frame[rows], want[rows])
        mine = np.concatenate([fr.Shard(k, nparts, R).global_rows(H) for k in (0, nparts - 1)]) if nparts > 1 else np.arange(H)
        others = np.setdiff1d(np.arange(H), mine)
        assert bool((frame[torch.from_numpy(others).cuda()] == -1.0).all())
        host = np.empty((H, W), np.float64)
        out = fr._capi.fr_output(None, host.ctypes.data, None, fr._capi.FR_MEM_HOST, fr._capi.FR_LAYOUT_FRAME)
        p = st.to_params(fr.FractalType.Mandelbrot, fr.Precision.F64)
        assert fr.lib().fr_render(renderer._ctx, C.byref(p), W, H, C.byref(out)) == fr._capi.FR_ERR_INVALID_ARG


def test_distinct_contexts_render_concurrently_from_host_threads(fr):
    """The header's threading contract: one fr_ctx is not re-entrant, distinct contexts may run concurrently.
    Four host threads, a context each (ctypes releases the GIL inside the calls), different views; every
    frame must be bit-identical to the same view rendered alone."""
    import threading
    import torch
    W, H = 384, 256
    views = [fr.FractalState(max_iterations=300 + 50 * k, center_x=-0.6 + 0.05 * k, zoom=2.5 - 0.3 * k) for k in range(4)]
    solo = []
    r0 = fr.Renderer(0)
    for st in views:
        nu = torch.empty((H, W), dtype=torch.float64, device="cuda:0")
        r0.render(st, W, H, nu=nu)
        solo.append(nu.clone())
    r0.close()
    results = [[] for _ in views]
    errors = []

    def worker(k):
        try:
            r = fr.Renderer(0)
            for _ in range(12):
                nu = torch.empty((H, W), dtype=torch.float64, device="cuda:0")
                rgba = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
                r.render(views[k], W, H, nu=nu, rgba=rgba)
                results[k].append(bool(torch.equal(nu, solo[k])))
            # an error in one thread must not leak into another thread's last-error string
            with pytest.raises(fr.FractalRendererError) as e:
                r.render(fr.FractalState(max_iterations=-k - 1), W, H, nu=nu)
            assert str(-k - 1) in str(e.value)
            r.close()
        except Exception as ex:      # noqa: BLE001
            errors.append((k, repr(ex)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(len(views))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errors, errors
    assert all(len(r) == 12 and all(r) for r in results), results


def test_overflow_of_a_survivor_stream_is_reported_not_swallowed(fr, oracle):
    """A survivor stream that runs out of blocks loses pixels.  The capacity is 1.5x the worst case, so it takes the
    tests-only option "debug_region_blocks" to get there -- and then the render must FAIL (FR_ERR_INTERNAL), in the
    synchronous call itself and, for an asynchronous render, at fr_ctx_check() / the next call; and the context must
    be usable again afterwards."""
    import torch
    r = fr.Renderer(0)
    try:
        st = fr.FractalState(max_iterations=1024, zoom=1.5)               # 60 % interior: most pixels survive the tile pass
        W, H = 512, 384
        nu = torch.empty((H, W), dtype=torch.float64, device="cuda:0")
        r.set_option("staging", 3)                                        # the two-launch schedule: the one with a stream in HBM
        r.render(st, W, H, nu=nu)
        good = nu.clone()
        r.set_option("debug_region_blocks", 1)                            # 8 regions x 1 block = 512 records
        with pytest.raises(fr.FractalRendererError) as e:
            r.render(st, W, H, nu=nu)
        assert e.value.status == fr._capi.FR_ERR_INTERNAL and "overflow" in str(e.value)
        s = torch.cuda.Stream()
        r.render(st, W, H, nu=nu, sync=False, stream=s.cuda_stream)       # asynchronous: nothing to report yet
        s.synchronize()
        with pytest.raises(fr.FractalRendererError) as e:
            r.check()
        assert e.value.status == fr._capi.FR_ERR_INTERNAL
        r.check()                                                          # reported once, then clear
        r.render(st, W, H, nu=nu, sync=False, stream=s.cuda_stream)
        s.synchronize()
        r.set_option("debug_region_blocks", 0)
        with pytest.raises(fr.FractalRendererError):                       # ... or it surfaces at the next call
            r.render(st, W, H, nu=nu)
        r.render(st, W, H, nu=nu)
        assert torch.equal(nu, good)
    finally:
        r.close()


def test_tile_pass_prologue_follows_the_viewport_back_to_back(fr):
    """The lean tile pass prepares its own control block and coordinate tables (lean_prologue_produce: written through to
    memory by its first workgroups, read by workgroups on every XCD after one wait).  Frames of DIFFERENT views, sizes,
    precisions and fractals enqueued back to back on one context with no host synchronisation in between -- small ones, whose
    tables and planes stay in the caches -- must equal the frames of a context that runs prepare_kernel as a launch of its
    own: a table entry, a queue head or a stream counter left over from the frame before would show."""
    import torch
    views = []
    for k in range(24):
        W, H = ((64, 64), (200, 120), (256, 256), (136, 72), (512, 304), (1000, 700))[k % 6]
        kw = dict(center_x=-0.5 + 0.07 * k, center_y=0.01 * (k % 5), zoom=3.0 / (1 + k % 7), max_iterations=(96, 300, 1024, 2048)[k % 4])
        ft = (fr.FractalType.Mandelbrot, fr.FractalType.JuliaSet, fr.FractalType.BurningShip)[k % 3]
        if ft == fr.FractalType.JuliaSet:
            kw.update(center_x=0.02 * k, julia_c_real=-0.8 + 0.01 * k, julia_c_imag=0.156)
        prec = fr.Precision.F64 if k % 2 else fr.Precision.F32
        views.append((fr.FractalState(**kw), W, H, ft, prec))
    planes = lambda W, H, prec: (torch.full((H, W, 4), -3.0, dtype=torch.float32, device="cuda:0"),
                                 torch.full((H, W), -3.0, dtype=torch.float64 if prec == fr.Precision.F64 else torch.float32, device="cuda:0"),
                                 torch.full((H, W), -3, dtype=torch.int32, device="cuda:0"))
    ref = fr.Renderer(0)
    r = fr.Renderer(0)
    try:
        ref.set_option("prepare", 1)
        want = []
        for st, W, H, ft, prec in views:
            rgba, nu, it = planes(W, H, prec)
            torch.cuda.synchronize()
            ref.render(st, W, H, fractal_type=ft, precision=prec, rgba=rgba, nu=nu, iter=it)
            want.append((rgba, nu, it))
        for rounds in range(3):
            got = [planes(W, H, prec) for _, W, H, _, prec in views]
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            for (st, W, H, ft, prec), (rgba, nu, it) in zip(views, got):
                r.render(st, W, H, fractal_type=ft, precision=prec, rgba=rgba, nu=nu, iter=it, sync=False, stream=side.cuda_stream)
            side.synchronize()
            r.check()
            for k, (w, g) in enumerate(zip(want, got)):
                for a, b in zip(w, g):
                    assert torch.equal(a, b), (rounds, k)
    finally:
        ref.close()
        r.close()


def test_tile_pass_prologue_epoch_wraps(fr):
    """The word the tile pass's workgroups wait on carries a 28-bit epoch (the context's count of such launches); near the end
    of that range the host clears the word behind the previous render and starts over.  Walked across the wrap here, one
    frame at a time and back to back: the renders must neither hang nor fail, the frames must be the separate launch's."""
    import torch
    W, H = 264, 136
    st = fr.FractalState(max_iterations=700, center_x=-0.743643887037151, center_y=0.13182590420533, zoom=0.02)
    ref = fr.Renderer(0)
    r = fr.Renderer(0)
    try:
        ref.set_option("prepare", 1)
        want = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
        ref.render(st, W, H, rgba=want)
        got = torch.empty_like(want)
        r.render(st, W, H, rgba=got)
        assert torch.equal(got, want)
        r.set_option("debug_prologue_epoch", 0x0FFFFFF0 - 3)              # three launches before the host starts over
        for k in range(8):
            got.fill_(-1.0)
            torch.cuda.synchronize()
            r.render(st, W, H, rgba=got)
            assert torch.equal(got, want), k
        # back to back across a second wrap, no host synchronisation in between
        r.set_option("debug_prologue_epoch", 0x0FFFFFF0 - 5)
        side = torch.cuda.Stream()
        outs = [torch.full_like(want, -1.0) for _ in range(12)]
        torch.cuda.synchronize()
        for o in outs:
            r.render(st, W, H, rgba=o, sync=False, stream=side.cuda_stream)
        side.synchronize()
        r.check()
        for k, o in enumerate(outs):
            assert torch.equal(o, want), k
    finally:
        ref.close()
        r.close()


def test_reserved_async_render_is_launch_only(fr, oracle):
    """The header's contract for fr_render_shard_async after fr_ctx_reserve: no allocation, no host synchronisation --
    shown the hard way, by capturing the call into a HIP graph (a hipMalloc / hipFree / stream synchronise inside a
    capture is an error) on a context that has never rendered, and replaying the graph."""
    import torch
    W, H = 1000, 700
    for kw, ft, prec, dt in ((dict(max_iterations=1024), fr.FractalType.Mandelbrot, fr.Precision.F64, torch.float64),
                             (dict(max_iterations=2048, center_x=0.0, julia_c_real=-0.8, julia_c_imag=0.156),
                              fr.FractalType.JuliaSet, fr.Precision.F32, torch.float32)):
        st = fr.FractalState(**kw)
        ref = fr.Renderer(0)
        want_nu = torch.empty((H, W), dtype=dt, device="cuda:0")
        want_rgba = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
        ref.render(st, W, H, fractal_type=ft, precision=prec, nu=want_nu, rgba=want_rgba)
        ref.close()
        r = fr.Renderer(0)
        try:
            r.reserve(st, W, H, fractal_type=ft, precision=prec)
            free0, _ = torch.cuda.mem_get_info()
            nu = torch.zeros_like(want_nu)
            rgba = torch.zeros_like(want_rgba)
            g = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            with torch.cuda.graph(g, stream=side):
                r.render(st, W, H, fractal_type=ft, precision=prec, nu=nu, rgba=rgba, sync=False,
                         stream=torch.cuda.current_stream().cuda_stream)
            for _ in range(3):
                nu.fill_(-1.0)
                rgba.fill_(-1.0)
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                assert torch.equal(nu, want_nu) and torch.equal(rgba, want_rgba)
                r.check()
            free1, _ = torch.cuda.mem_get_info()
            assert free0 - free1 < (4 << 20)            # the graph's own bookkeeping, no scratch growth
            del g
        finally:
            r.close()


def test_export_is_ordered_behind_a_render_on_the_callers_stream(fr):
    """fr_export_rgb8 runs on the context's own (non-blocking) stream; the render that produced its input may have been
    enqueued on a caller's stream.  The export must wait for it: no host synchronisation in between here."""
    import torch
    W = H = 2048
    st = fr.FractalState(max_iterations=1024, zoom=1.5)                   # ~0.6 ms of rendering
    r = fr.Renderer(0)
    try:
        rgba = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
        r.render(st, W, H, rgba=rgba)
        want8 = r.export_rgb8(rgba, W, H, through_half=True).clone()
        want16 = r.export_rgb16(rgba, W, H).clone()
        user = torch.cuda.Stream()
        for _ in range(5):
            with torch.cuda.stream(user):
                rgba.zero_()
            r.render(st, W, H, rgba=rgba, sync=False, stream=user.cuda_stream)
            got8 = r.export_rgb8(rgba, W, H, through_half=True)            # context stream, behind ev_end of the render
            assert torch.equal(got8, want8)
            with torch.cuda.stream(user):
                rgba.zero_()
            r.render(st, W, H, rgba=rgba, sync=False, stream=user.cuda_stream)
            got16 = torch.empty_like(want16)
            r.export_rgb16(rgba, W, H, out=got16, stream=user.cuda_stream)  # the _async form on the producing stream
            user.synchronize()
            assert torch.equal(got16, want16)
    finally:
        r.close()


def test_tolerance_exceptions_stay_rare():
    """Last test of the file: over everything check_against looked at in this session, the pixels accepted through a
    tolerance exception (fp32 palette wrap, pre-gamma comparison next to black) stay below 0.1 %."""
    if EXCEPTIONS["pixels"] == 0:
        pytest.skip("no parity check ran in this session")
    frac = (EXCEPTIONS["wrap"] + EXCEPTIONS["pre_gamma"]) / EXCEPTIONS["pixels"]
    print("tolerance exceptions: %d palette-wrap + %d pre-gamma of %d pixels (%.2e); worst single frame %.2e"
          % (EXCEPTIONS["wrap"], EXCEPTIONS["pre_gamma"], EXCEPTIONS["pixels"], frac, EXCEPTIONS["worst_call"]))
    assert frac < EXCEPTION_CAP
