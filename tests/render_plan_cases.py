"""The requests of tests/golden/render_plans.npz: every render whose schedule test_render_plan_host.py pins.

A case is a tuple (fractal, f64, max_iter, aa, trap, stripe, interior_style, W, H, part, nparts, rows_per_strip,
compute_units, tunings) -- nparts 0: no shard; tunings: "name=value,name=value" for fr_plan_describe.  The matrix straddles
every threshold the planner names (fractalrenderer_amd/csrc/fr_plan.h): staging_threshold's pixel counts and max_iter
values, plan_stages' budget clamps, the bounded / moderate limits, the shard and grid rules of plan_tile_queue, the lean
predicates, the SSAA routes, and every tuning that enters the plan, one at a time ("prepare" and "mandelbulb_split" do not:
begin_frame and enqueue_mandelbulb read them from the context).
"""
from __future__ import annotations

import itertools

MANDELBROT, JULIA, BURNING_SHIP, DEEP_ZOOM = 0, 1, 2, 5
FRACTALS = (MANDELBROT, JULIA, BURNING_SHIP)

# max_iter around every staging threshold of staging_threshold()
STAGING_ITERS = [m + d for m in (256, 384, 512, 768, 1024, 1536) for d in (-1, 0, 1)]

# one tuning at a time, each at values other than its automatic choice (and at the edges of what its setter does)
SINGLE_TUNINGS = [
    "workgroups_per_cu=3", "workgroups_per_cu=16", "run_max=16", "run_min=8", "run_min=64,run_max=16", "shift_bias=2",
    "shift_bias=-2", "shift_bias=16", "shift_bias=-16", "subtile_shape=3", "subtile_shape=4", "subtile_shape=6",
    "pool_refill_at=8", "pool_refill_at=64", "stage_first=48", "stage_first=100", "stream_run_max=4", "stream_run_min=2",
    "stream_run_min=2,stream_run_max=4", "stream_workgroups_per_cu=2", "probes=3", "probes=31", "stream_probes=2",
    "stream_rotate=1", "stream_rotate=2", "regions=8", "regions=64", "tile_pixels=1", "tile_pixels=2",
    "tile_exit=1", "tile_exit=100", "tile_exit_from=48", "ssaa=1", "ssaa=2", "stripes=1", "ssaa_band_samples=100000",
    "pool_items_per_wg=8", "pool_items_per_wg=4096", "debug_region_blocks=3", "periodicity=-1",
    "periodicity=1", "periodicity=100", "staging=1", "staging=2", "staging=3", "shards=8", "shards=64", "tile_kernel=1",
]


def _case(fractal=MANDELBROT, f64=0, max_iter=256, aa=1, trap=0, stripe=0, interior=0, W=64, H=64, shard=(0, 0, 0), cu=256,
          tunings=""):
    return (fractal, f64, max_iter, aa, trap, stripe, interior, W, H, shard[0], shard[1], shard[2], cu, tunings)


def cases():
    out = []
    # A. pixel counts just below, at and just above 2^18 .. 2^24: one row less / more, and one pixel less / more (a one-row frame)
    for k, w in ((18, 512), (19, 1024), (20, 1024), (23, 4096), (24, 4096)):
        n = 1 << k
        frames = [(w, n // w - 1), (w, n // w), (w, n // w + 1), (n - 1, 1), (n + 1, 1)]
        for (W, H), fractal, f64, mi in itertools.product(frames, FRACTALS, (0, 1), STAGING_ITERS):
            out.append(_case(fractal, f64, mi, W=W, H=H))
    # B. max_iter: the bounded (128 / aa^2) and moderate (768 / aa^2) limits, the clamps of max_iter / 28 and max_iter / 11, 2^24
    budget_iters = [m + d for m in (896, 1120, 1568, 5376, 5600, 1056, 1144, 2024, 2200) for d in (-1, 0, 1)] + [2048, 4096, 16384, 1 << 24]
    for (W, H), f64, mi in itertools.product(((1920, 1080), (4096, 4096), (4097, 4096), (8192, 8192)), (0, 1), budget_iters):
        out.append(_case(MANDELBROT, f64, mi, W=W, H=H))
        out.append(_case(MANDELBROT, f64, mi, W=W, H=H, tunings="periodicity=-1"))
    for aa, f64, fractal in itertools.product((1, 2, 3), (0, 1), FRACTALS):
        for mi in sorted({128 // (aa * aa) + d for d in (-1, 0, 1, 2)} | {768 // (aa * aa) + d for d in (-1, 0, 1, 2)}):
            for t in ("", "ssaa=1"):
                out.append(_case(fractal, f64, mi, aa=aa, W=1920, H=1080, tunings=t))
    # C. forced staging: 2 * stage_first +- 1, budgets that are no multiple of the unchecked block, staging = 3 around 2 * 32,
    #    and on an fp64 frame of 2^24 pixels, where the pool that runs everything has the longer budget
    for sf, f64 in itertools.product((8, 48, 64, 100, 192, 1000), (0, 1)):
        for d in (-1, 0, 1):
            out.append(_case(MANDELBROT, f64, 2 * sf + d, W=1920, H=1080, tunings=f"stage_first={sf}"))
            out.append(_case(JULIA, f64, 2 * sf + d, W=512, H=512, tunings=f"stage_first={sf}"))
    for (W, H), f64, mi in itertools.product(((1920, 1080), (4096, 4096)), (0, 1), (17, 31, 32, 33, 63, 64, 65, 100, 191, 192, 193, 383, 384, 385)):
        out.append(_case(MANDELBROT, f64, mi, W=W, H=H, tunings="staging=3"))
        # (fp64, 2^24 pixels, max_iter below 2 x 96: plan_stages answers ONE pass for the pool that runs everything out while the
        # render stays two passes -- nstages 2, nstages_all 1; enqueue_render then clears one stage's control words, as it always has)
        out.append(_case(MANDELBROT, f64, mi, W=W, H=H, tunings="staging=3,periodicity=-1"))
        out.append(_case(MANDELBROT, f64, mi, W=W, H=H, tunings="stage_first=16,periodicity=-1"))
    # D. frame shapes: 1x1, widths that are / are not powers of two (nsx_shift), fewer sub-tiles than 4 x run_min
    shapes = [(1, 1), (7, 3), (8, 8), (9, 9), (16, 8), (24, 16), (64, 64), (65, 64), (64, 65), (128, 8), (257, 129), (520, 504),
              (512, 512), (1000, 1000), (1024, 768), (2048, 64), (3000, 17)]
    for (W, H), fractal, f64, mi in itertools.product(shapes, FRACTALS, (0, 1), (64, 256, 2048)):
        out.append(_case(fractal, f64, mi, W=W, H=H))
    # E. every combination needs_effects() looks at, with the tunings that decide between the effects variant and lean stripes
    for (W, H), fractal, trap, stripe, interior, aa, mi, t in itertools.product(
            ((520, 504), (1920, 1080)), FRACTALS, (0, 1), (0, 1), (0, 1, 2, 3), (1, 2), (256, 2048),
            ("", "stripes=1", "tile_pixels=1", "tile_kernel=1", "subtile_shape=4")):
        out.append(_case(fractal, 0, mi, aa=aa, trap=trap, stripe=stripe, interior=interior, W=W, H=H, tunings=t))
    for trap, stripe, interior in itertools.product((0, 1), (0, 1), (0, 2, 3)):
        out.append(_case(MANDELBROT, 1, 2048, trap=trap, stripe=stripe, interior=interior, W=1920, H=1080))
    # F. shards: rows_per_strip a multiple of 8, not one, and one only after the multiplication by aa
    shards = [(0, 1, 0), (0, 2, 0), (1, 2, 8), (0, 2, 12), (1, 3, 4), (0, 2, 4), (1, 4, 16), (7, 8, 0), (2, 8, 20), (0, 2, 1080)]
    for sh, fractal, f64, aa, mi, stripe in itertools.product(shards, (MANDELBROT, JULIA), (0, 1), (1, 2, 3), (256, 2048), (0, 1)):
        if stripe and fractal != MANDELBROT:
            continue
        out.append(_case(fractal, f64, mi, aa=aa, stripe=stripe, W=1920, H=1080, shard=sh))
    # G. SSAA routes: sample grids below, at and above "ssaa_band_samples"; bands that do not divide H; a band below one
    #    sub-tile row of samples; 2^31 samples; sharded frames above the cap
    for aa, band in itertools.product((2, 3), (1 << 20, 520 * 504 * 4, 520 * 504 * 4 - 1, 520 * 504 * 9, 520 * 504 * 9 - 1, 200000, 16640, 16639, 10000)):
        for mi, f64 in itertools.product((256, 2048), (0, 1)):
            out.append(_case(MANDELBROT, f64, mi, aa=aa, W=520, H=504, tunings=f"ssaa_band_samples={band}"))
            out.append(_case(JULIA, f64, mi, aa=aa, W=520, H=504, shard=(1, 2, 8), tunings=f"ssaa_band_samples={band}"))
    for (W, H), aa, t in itertools.product(((16384, 32768), (16384, 32767), (8192, 8192), (23171, 23171), (4096, 4096)), (2, 3),
                                           ("", "ssaa=2", "ssaa=1", "ssaa=2,ssaa_band_samples=1048576")):
        out.append(_case(MANDELBROT, 1, 1024, aa=aa, W=W, H=H, tunings=t))
        out.append(_case(MANDELBROT, 1, 1024, aa=aa, W=W, H=H, shard=(0, 2, 8), tunings=t))
    # H. 8 compute units: grids below the number of shards, lane-pool grids below 64
    for (W, H), fractal, f64, aa, mi in itertools.product(((64, 64), (520, 504), (1920, 1080), (4096, 4096)), (MANDELBROT, JULIA),
                                                          (0, 1), (1, 2), (64, 256, 2048)):
        out.append(_case(fractal, f64, mi, aa=aa, W=W, H=H, cu=8))
        out.append(_case(fractal, f64, mi, aa=aa, W=W, H=H, cu=8, tunings="shards=64"))
    # I. every tuning that enters the plan, one at a time, on renders of every route and family
    bases = [dict(f64=0, max_iter=2048, W=1920, H=1080), dict(f64=1, max_iter=2048, W=1920, H=1080),
             dict(f64=0, max_iter=256, W=1920, H=1080), dict(f64=1, max_iter=1024, W=4096, H=4096),
             dict(f64=0, max_iter=2048, aa=2, W=520, H=504), dict(f64=0, max_iter=2048, stripe=1, W=1920, H=1080),
             dict(fractal=JULIA, f64=0, max_iter=512, W=257, H=129), dict(fractal=BURNING_SHIP, f64=1, max_iter=4096, trap=1, W=520, H=504),
             dict(f64=0, max_iter=2048, W=1920, H=1080, shard=(1, 2, 12)), dict(f64=1, max_iter=2048, W=64, H=64, cu=8)]
    for base, t in itertools.product(bases, SINGLE_TUNINGS):
        out.append(_case(tunings=t, **base))
    # J. Deep_Zoom: routed before anything else is decided
    for mi, aa, sh in itertools.product((256, 4096), (1, 2), ((0, 0, 0), (1, 2, 8))):
        out.append(_case(DEEP_ZOOM, 0, mi, aa=aa, W=520, H=504, shard=sh))
    return out


def parse_tunings(text: str):
    return [(kv.split("=")[0], int(kv.split("=")[1])) for kv in text.split(",") if kv]
