"""The Deep_Zoom loop-structure cases of test_deepzoom_gpu.py as data, and the CPU predicates that say what each can see.

A case is a tuple (OracleParams, W, H), as in cases.py.  deep_zoom_kernel (fr_kernels.hip.h) runs two phases: it perturbs
against orbit[0 .. n_ref), n_ref = min(ref_iter, max_iter), then iterates in plain fp32 over [n_ref, max_iter) from
orbit[ref_iter - 1] + dz (from c when there is no orbit).  Each phase is a loop over groups of four updates behind a wave-wide
"anybody alive" ballot, followed by a tested tail.  The groups below put escapes where each of those parts decides the result:

  REMAINDER        perturbed, escaping centre: one centre per L % 4 (L the orbit length), max_iter = L + 0..7 -- every pair
                   (n_ref % 4, plain length % 4), with and without a full group of four in the plain phase
  INTERIOR_CENTRE  perturbed, the orbit as long as max_iter = 1..9: no plain phase, n_ref % 4 takes every value
  NO_ORBIT         use_perturbation = 0: the plain phase alone, from z = c at k = 0
  RAGGED           frames that are no multiple of the 8x8 sub-tile: lanes without a sample start dead next to live ones
  WAVE_EXIT        whole sub-tiles dead before the last group of four (the break, the skipped tails) next to sub-tiles that
                   run to the end, and sub-tiles that are wholly interior
  COLOUR           palette_mode -1..4 x (color_scale, color_offset) x bailout 0.5 (the clamp to 2) .. 3e19 (bailout^2 = inf)
  SWEEP            a seeded sweep over views, iteration budgets, bailouts, palettes, ragged sizes and row-strip shards

The predicates work on the CPU oracle's output only (test_deepzoom_cases_host.py asserts them for every case); whether a
GPU comparison means anything is decided there, on the CPU, never by the GPU test about itself.
"""
from __future__ import annotations

import functools
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from cases import SEAHORSE  # noqa: E402

F32 = np.float32
GROUP = 4                       # updates per ballot in both phases of deep_zoom_kernel
TILE = 8                        # one wave = one 8x8 sub-tile (the default sub-tile shape)
WRAP_EPS = 1e-4                 # check_against's distance from the fract() wrap
W0, H0 = 72, 40


def dz(**kw):
    return O.OracleParams(fractal=5, precision=0, **kw)


# ---- the views -----------------------------------------------------------------------------------------------------------
# escaping centres, one per L % 4: (view, L)
REMAINDER_VIEWS = {0: (dict(center_x=-1.228, center_y=-0.245, zoom=10.0), 12),
                   1: (dict(center_x=0.548, center_y=-0.059, zoom=2.5), 5),
                   2: (dict(center_x=0.458, center_y=0.005, zoom=2.5), 6),
                   3: (dict(center_x=0.328, center_y=0.707, zoom=2.5), 7)}
INTERIOR_VIEW = dict(center_x=-0.1, center_y=0.65, zoom=20.0)
NO_ORBIT_VIEW = dict(center_x=-0.6, center_y=0.2, zoom=25.0)
WAVE_EXIT_VIEW = dict(center_x=-0.75, center_y=0.1, zoom=100.0)
NO_ORBIT_ITERS = tuple(range(1, 10)) + (15, 16, 17)
RAGGED_SIZES = ((9, 9), (65, 7), (1, 1), (3, 70), (131, 67))


def remainder(m, max_iter, **kw):
    return dz(max_iterations=max_iter, use_perturbation=1, **REMAINDER_VIEWS[m][0], **kw)


def no_orbit(max_iter, **kw):
    return dz(max_iterations=max_iter, use_perturbation=0, **NO_ORBIT_VIEW, **kw)


def interior_centre(max_iter, **kw):
    return dz(max_iterations=max_iter, use_perturbation=1, **INTERIOR_VIEW, **kw)


REMAINDER = {f"L{m}-r{r}": (remainder(m, L + r), W0, H0)
             for m, (_, L) in REMAINDER_VIEWS.items() for r in range(8)}

INTERIOR_CENTRE = {f"mi{mi}": (interior_centre(mi), W0, H0) for mi in range(1, 10)}

NO_ORBIT = {f"mi{mi}": (no_orbit(mi), W0, H0) for mi in NO_ORBIT_ITERS}

RAGGED = {f"{name}-{W}x{H}": (p, W, H)
          for (name, p), (W, H) in itertools.product((("L3-r5", remainder(3, 12)), ("no_orbit-17", no_orbit(17))), RAGGED_SIZES)}

WAVE_EXIT = {"escaping-37": (dz(max_iterations=37, use_perturbation=1, **WAVE_EXIT_VIEW), 64, 64),
             "interior-9": (interior_centre(9), 64, 64)}

# ---- COLOUR ---------------------------------------------------------------------------------------------------------------
PALETTES = (-1, 0, 1, 2, 3, 4)
BAILOUTS = (0.5, 2.0, 4.0, 1e4, 3e19)
SCALE_OFFSET = ((1.0, 0.0), (-2.5, 0.3), (6.0, 0.9), (0.0, 0.5))
# The no-orbit view is full of samples that leave in the first update with nu next to 0: with the offsets above up to 12 of
# its 2880 samples sit within WRAP_EPS of a palette's wrap, more than check_against's exception lets pass (near_wrap below).
# Its offsets are moved until no combination holds more than 1 (-1.5: t < 0 for every sample, fract of a negative argument).
COLOUR_VIEWS = {"L1-12": (lambda **kw: remainder(1, 12, **kw), SCALE_OFFSET),
                "no_orbit-17": (lambda **kw: no_orbit(17, **kw), ((1.0, 0.55), (-2.5, -1.5), (6.0, 0.95), (0.0, 0.5)))}


def colour_id(view, palette, scale, offset, bailout):
    return f"{view}-p{palette}-s{scale:g}-o{offset:g}-b{bailout:g}"


COLOUR_KEYS = {colour_id(view, pal, sc, off, b): (view, pal, sc, off, b)
               for view, (_, pairs) in COLOUR_VIEWS.items() for pal, (sc, off), b in itertools.product(PALETTES, pairs, BAILOUTS)}
COLOUR = {cid: (COLOUR_VIEWS[view][0](palette_mode=pal, color_scale=sc, color_offset=off, bailout=b), W0, H0)
          for cid, (view, pal, sc, off, b) in COLOUR_KEYS.items()}

# ---- SWEEP ----------------------------------------------------------------------------------------------------------------
SWEEP_SEED = 20261022
SWEEP_TRIALS = 32
SWEEP_ITERS = (1, 2, 3, 5, 6, 7, 9, 33, 34, 35, 63, 64)
SWEEP_BAILOUTS = (1.0, 2.0, 2.5, 4.0, 16.0, 1000.0)
# the Mandelbrot boundary anchors of test_randomised_views_match_the_oracle, and the four REMAINDER centres
SWEEP_ANCHORS = ((-0.743643887037151, 0.13182590420533), (-0.1011, 0.9563), (-1.25066, 0.02012), (0.275, 0.0), (-0.5, 0.0),
                 (-1.7497, 0.00001)) + tuple((v["center_x"], v["center_y"]) for v, _ in REMAINDER_VIEWS.values())


def _sweep():
    """{id: (OracleParams, W, H, shard)}, shard = None or (part, nparts, rows_per_strip)"""
    rng = np.random.default_rng(SWEEP_SEED)
    out = {}
    for trial in range(SWEEP_TRIALS):
        ax, ay = SWEEP_ANCHORS[int(rng.integers(0, len(SWEEP_ANCHORS)))]
        height = float(10.0 ** rng.uniform(-3.0, 0.5))                 # of the view, in c-units
        W, H = int(rng.integers(9, 132)), int(rng.integers(5, 68))
        p = dz(center_x=ax + height * float(rng.uniform(-0.2, 0.2)), center_y=ay + height * float(rng.uniform(-0.2, 0.2)),
               zoom=height * H / 4.0,                                   # the shader's view is 4 * zoom / H high
               max_iterations=int(rng.choice(SWEEP_ITERS)), use_perturbation=int(rng.integers(0, 2)),
               palette_mode=int(rng.integers(-1, 5)), bailout=float(rng.choice(SWEEP_BAILOUTS)),
               color_offset=float(F32(rng.uniform(0, 1))), color_scale=float(F32(rng.uniform(0.5, 6))))
        shard = None
        if trial % 3 == 1:
            nparts = int(rng.integers(2, 6))
            part, R = int(rng.integers(0, nparts)), int(rng.integers(1, 9))
            shard = (part % min(nparts, -(-H // R)), nparts, R)         # a part that owns rows: one of the first strips'
        out[f"trial{trial:02d}"] = (p, W, H, shard)
    return out


SWEEP = _sweep()

GROUPS = {"remainder": REMAINDER, "interior_centre": INTERIOR_CENTRE, "no_orbit": NO_ORBIT, "ragged": RAGGED,
          "wave_exit": WAVE_EXIT, "colour": COLOUR, "sweep": {k: v[:3] for k, v in SWEEP.items()}}

# ---- beyond single frames -------------------------------------------------------------------------------------------------
SEAHORSE_SIZE = (203, 131)


def seahorse(max_iter):
    """cases.py's deepzoom_seahorse view at another iteration budget, in palette 1.  Not in palette 0: the shader takes
    fract(t * 0.05) of t = nu * color_scale + color_offset in float, and from nu = 1280 on one ulp of t * 0.05 >= 64 is
    7.6e-6, which the hsv ramp (slope 6 * 0.8 * 0.9 = 4.32) turns into 3.3e-5 of colour -- above RGB_TOL for every sample
    whose nu = iter + 1 - log2(log|z| / log 2) rounds the other way under another logf, about one sample in a thousand at
    these magnitudes (measured on the 203 x 131 frame at max_iter 2000: 7 samples, 3.3021e-05 each, nu within its bar).
    Palette 1 is a mix of slope <= 1 over fract(t * 0.03): one ulp of t * 0.03 <= 123 is 7.6e-6 of colour, under the bar."""
    return dz(center_x=SEAHORSE[0], center_y=SEAHORSE[1], zoom=1e-6, max_iterations=max_iter, use_perturbation=1, palette_mode=1)


# rendered in this order on one context: a long orbit, short ones behind it, no orbit at all, a longer one that grows the
# buffers, and the first short one again
ORBIT_SEQUENCE = ((seahorse(2000),) + SEAHORSE_SIZE, (remainder(1, 12), W0, H0), (no_orbit(17), W0, H0), (remainder(3, 14), W0, H0),
                  (seahorse(4096),) + SEAHORSE_SIZE, (remainder(1, 12), W0, H0))

ENTRY_POINT_CASES = {"L3-r5": (remainder(3, 12), W0, H0), "no_orbit-17": (no_orbit(17), W0, H0)}


# ---- the reference and what it shows --------------------------------------------------------------------------------------
def _key(case):
    p, W, H = case
    return (tuple(sorted(p.__dict__.items())), W, H)


@functools.lru_cache(maxsize=None)
def _render(key):
    ref = O.render(O.OracleParams(**dict(key[0])), key[1], key[2])
    for a in (ref.rgba, ref.nu, ref.iter):
        a.setflags(write=False)
    return ref


def reference(case):
    """oracle.render of a case, computed once and read-only"""
    return _render(_key(case))


def orbit_length(p, max_iter=10000):
    """L: the length of the reference orbit of p's centre, uncapped (the issue's L)"""
    return len(O.reference_orbit(p.center_x, p.center_y, max_iter))


def ref_iter(p):
    """reference_iterations as the host computes it for this render: 0 without perturbation, else capped at max_iter"""
    return orbit_length(p, p.max_iterations) if p.use_perturbation else 0


def n_ref(p):
    return min(ref_iter(p), p.max_iterations)


def perturbed_tail(p):
    """the indices of the perturbed phase's tested tail, after its last full group of four"""
    n = n_ref(p)
    return range(GROUP * (n // GROUP), n)


def plain_phase(p):
    return range(n_ref(p), p.max_iterations)


def escapes_at(it, i):
    return int((it == i).sum())


def interior(it, p):
    return int((it == p.max_iterations).sum())


def near_wrap(p, nu):
    """the samples check_against would let through its palette-wrap exception: its formula for fractal 5, on the reference"""
    scale, off = F32(p.color_scale), F32(p.color_offset)
    t = (nu.astype(F32) * scale + off) * F32({0: 0.05, 1: 0.03, 2: 0.04}.get(p.palette_mode, 0.02))
    u = t - np.floor(t)
    return int((np.minimum(u, 1 - u) < WRAP_EPS).sum())


def colour_ulp(p):
    """What one ulp of a palette's fract argument t * k is worth in colour at the largest nu of a frame (nu <= max_iter + 1,
    t = nu * color_scale + color_offset): the float rounding of t * k alone moves a colour by this much when nu differs by
    an ulp between two logf.  Slope of the palette over fract: 6 * 0.8 * 0.9 for the hsv ramp, at most 1 for the mixes."""
    k, slope = {0: (0.05, 4.32), 1: (0.03, 1.0), 2: (0.04, 0.9)}.get(p.palette_mode, (0.02, 1.0))
    t = abs(p.color_scale) * (p.max_iterations + 1) + abs(p.color_offset)
    return float(np.spacing(F32(t * k))) * slope


def wrap_cap(npix):
    """check_against's cap on the exceptions of one frame"""
    return max(2, 1e-3 * npix)


def blocks(it):
    """the aligned full 8x8 blocks of an iter plane, (n, 64)"""
    H, W = it.shape
    h, w = H // TILE * TILE, W // TILE * TILE
    return it[:h, :w].reshape(h // TILE, TILE, w // TILE, TILE).transpose(0, 2, 1, 3).reshape(-1, TILE * TILE)


def block_census(case):
    """(dead early, mixed, all interior) aligned 8x8 blocks: fully escaped before the last full group of the perturbed phase
    starts (the wave takes the break there, skips the tail and takes the plain phase's break at once); holding both an escape
    in the first group and a sample that reaches the last group; wholly interior"""
    p = case[0]
    b = blocks(reference(case).iter)
    last_group = GROUP * (n_ref(p) // GROUP) - GROUP
    dead = int((b.max(axis=1) < last_group).sum())
    mixed = int(((b.min(axis=1) < GROUP) & (b.max(axis=1) >= last_group)).sum())
    inside = int((b.min(axis=1) == p.max_iterations).sum())
    return dead, mixed, inside
