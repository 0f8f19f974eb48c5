"""The Phoenix orbit-loop cases of test_phoenix_orbit_gpu.py as data, and the CPU predicates that say what each can see.

A case is a tuple (W, H, kwargs for phoenix_ref.render), f64 among the kwargs.  phoenix_orbit (fr_phoenix.hip.h) runs blocks
of 16 updates unchecked, replays a block in which a lane went past 4 with the test after every update, parks escaped lanes
at z = z_prev = C = 0 and finishes the last max_iter % 16 updates in a tested loop; the groups below put escapes where each
of those parts decides the result:

  BOUNDARY   max_iter around every multiple of 16 up to 63, on a view whose tail holds escapes at every one of them
  REENTRY    views on which orbits, continued past their first escape, come back to |z|^2 <= 4 inside the same block
  RAGGED     frames that are no multiple of the 8x8 sub-tile: lanes without a sample run next to live ones
  COLOUR_F64 the fp64 kernel's narrowing into the float colour stage: supersampling x post chain x stripe density
  JULIA_F64  Julia mode (C = julia_c for every pixel) in fp64
  INTERIOR   the reference fixture's interior view: lastZ of samples that never escape, read after the tail

The predicates work on phoenix_ref output only (test_phoenix_host.py::test_orbit_cases_can_fail asserts them for every case);
whether a GPU comparison means anything is decided there, on the CPU, never by the GPU test about itself.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

import phoenix_ref

F32 = np.float32
BLOCK = 16                      # kPhoenixBlock, fr_phoenix.hip.h
WRAP_EPS = 1e-4

W0, H0 = 72, 40
CLASSIC = dict(phoenix_p=0.0, phoenix_r=-0.5)
SWIRL = dict(phoenix_p=0.2, phoenix_r=-0.3)
CHAOS = dict(phoenix_p=0.3, phoenix_r=-0.6)
PARAMS = {"classic": CLASSIC, "swirl": SWIRL, "chaos": CHAOS}
TAIL_VIEW = dict(center_x=-0.45, center_y=0.55, zoom=0.4)      # escapes in the tail at every BOUNDARY_ITERS, both parameter sets
SWIRL_VIEW = dict(center_x=-0.3, center_y=0.0, zoom=2.5)
INTERIOR_VIEW = dict(center_x=0.0, center_y=0.0, zoom=0.6)
JULIA_C = ((float(F32(-0.7)), float(F32(0.27015))), (0.6, 0.55))

BOUNDARY_ITERS = (15, 16, 17, 31, 32, 33, 47, 48, 49, 63)
POSTS = {"linear": dict(post=False),
         "post": dict(post=True, color_brightness=1.2, color_saturation=0.8, color_contrast=1.1),
         "post_floors": dict(post=True, color_brightness=0.02, color_saturation=-1.0, color_contrast=0.0)}
DENSITIES = (0.0, 0.005, 10.0, 17.5)


def _case(W=W0, H=H0, **kw):
    return (W, H, kw)


BOUNDARY = {f"{name}-{mi}-{'f64' if f64 else 'f32'}": _case(max_iterations=mi, f64=f64, **TAIL_VIEW, **PARAMS[name])
            for mi, f64, name in itertools.product(BOUNDARY_ITERS, (False, True), ("classic", "chaos"))}

REENTRY = {f"{name}-{mi}-{'f64' if f64 else 'f32'}": _case(max_iterations=mi, f64=f64, **view, **PARAMS[name])
           for (name, view), mi, f64 in itertools.product((("swirl", SWIRL_VIEW), ("chaos", {})), (49, 64), (False, True))}

RAGGED = {f"{W}x{H}-{'f64' if f64 else 'f32'}": _case(W, H, max_iterations=33, f64=f64, **TAIL_VIEW, **CHAOS)
          for (W, H), f64 in itertools.product(((9, 9), (65, 7), (1, 1)), (False, True))}

COLOUR_F64 = {f"{mi}-aa{aa}-{post}-d{dens}": _case(max_iterations=mi, f64=True, aa=aa, stripe_density=dens, **TAIL_VIEW,
                                                    **POSTS[post])
              for mi, aa, post, dens in itertools.product((33, 80), (1, 2, 3), POSTS, DENSITIES)}

# a Julia-mode frame is one colour: the reference is 4x4, the GPU frame as large as the test likes
JULIA_F64 = {f"jc{k}-{mi}-{post}": _case(4, 4, max_iterations=mi, f64=True, use_julia_set=True, julia_c_real=jc[0],
                                         julia_c_imag=jc[1], post=(post == "post"))
             for (k, jc), mi, post in itertools.product(enumerate(JULIA_C), (17, 128), ("linear", "post"))}

INTERIOR = {f"{mi}-{'f64' if f64 else 'f32'}": _case(max_iterations=mi, f64=f64, stripe_density=10.0, **INTERIOR_VIEW)
            for mi, f64 in itertools.product((33, 47), (False, True))}

GROUPS = {"boundary": BOUNDARY, "reentry": REENTRY, "ragged": RAGGED, "colour_f64": COLOUR_F64, "julia_f64": JULIA_F64,
          "interior": INTERIOR}


def _key(case):
    W, H, kw = case
    return (W, H, tuple(sorted(kw.items())))


@functools.lru_cache(maxsize=None)
def _traced(key):
    """phoenix_ref.render of a case, with what it hands to orbit() and colour() for every supersample recorded: the map
    from pixel to C and from the orbit to the palette argument is render's own, not restated here."""
    W, H, kw = key[0], key[1], dict(key[2])
    orbits, colours = [], []
    orbit0, colour0 = phoenix_ref.orbit, phoenix_ref.colour

    def orbit(cx, cy, p, r, max_iter, T):
        out = orbit0(cx, cy, p, r, max_iter, T)
        orbits.append((cx.copy(), cy.copy(), p, r, max_iter, T) + tuple(out))
        return out

    def colour(t, smooth, ezx, ezy, density):
        colours.append((t.copy(), smooth.copy(), ezx.copy(), ezy.copy(), density))
        return colour0(t, smooth, ezx, ezy, density)

    phoenix_ref.orbit, phoenix_ref.colour = orbit, colour
    try:
        planes = phoenix_ref.render(W, H, **kw)
    finally:
        phoenix_ref.orbit, phoenix_ref.colour = orbit0, colour0
    for a in planes:
        a.setflags(write=False)
    return planes, orbits, colours


def reference(case):
    """(iter, smooth, rgb) of phoenix_ref.render, computed once per case and read-only"""
    return _traced(_key(case))[0]


def tail_escapes(it, max_iter):
    """samples whose escape falls into the tested tail after the last full block"""
    return int(((it >= BLOCK * (max_iter // BLOCK)) & (it < max_iter)).sum())


def last_update_escapes(it, max_iter):
    """samples that escape in the very last update: the only ones a loop that stops one update early gets wrong"""
    return int((it == max_iter - 1).sum())


def block_escapes(it, max_iter):
    """escapes in each full block of 16 updates"""
    return [int(((it >= b) & (it < b + BLOCK)).sum()) for b in range(0, BLOCK * (max_iter // BLOCK), BLOCK)]


def reentering(case):
    """Mask (H, W) of the (0,0) samples whose orbit, continued WITHOUT the break, returns to |z|^2 <= 4 before the end of the
    16-block that holds its first escape: the samples the running maximum of the unchecked block exists for."""
    W, H, _ = case
    planes, orbits, _ = _traced(_key(case))
    cx, cy, p, r, max_iter, T, it = orbits[0][:7]
    zx = np.zeros(cx.size, T); zy = np.zeros(cx.size, T); qx = np.zeros(cx.size, T); qy = np.zeros(cx.size, T)
    cx, cy = cx.astype(T), cy.astype(T)
    p, r, two, four = T(p), T(r), T(2.0), T(4.0)
    first = np.full(cx.size, -1, np.int64)
    back = np.zeros(cx.size, bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(max_iter + BLOCK):
            x = (((zx * zx - zy * zy) + cx) + r * qx) + p * zx          # as phoenix_ref.orbit writes its update
            y = ((((two * zx) * zy) + cy) + r * qy) + p * zy
            qx, qy, zx, zy = zx, zy, x, y
            d = zx * zx + zy * zy
            out = d > four
            first = np.where((first < 0) & out & (i < max_iter), i, first)
            block_end = BLOCK * (first // BLOCK + 1)
            back |= (first >= 0) & (i > first) & (i < block_end) & (d <= four)
    assert np.array_equal(np.where(first < 0, max_iter, first), it)     # the same first escape as the reference's loop
    return back.reshape(H, W)


def reentries(case):
    return int(reentering(case).sum())


def near_wrap(case):
    """Samples for which an argument of a fract in phoenix_ref.colour / fire lies within WRAP_EPS of an integer: t after the
    pow, and t + 0.1 * mod when the stripes are on.  The palette is continuous at its knots; the wrap is its only jump, so the
    only place where one ulp of the GPU's libm can flip a colour.  Samples with the exact interior value t == 1 are excluded:
    t is then the same float on both sides (pow(1, 0.8) == 1, fract(1) == 0), and t + 0.1 * mod with mod = 0.5 + 0.5 * sin(..)
    >= 0 in any libm stays in [1, 1.1], on one side of the wrap."""
    _, _, colours = _traced(_key(case))
    n = 0
    for t, smooth, ezx, ezy, density in colours:
        with np.errstate(invalid="ignore"):
            t = np.power(t.astype(F32), F32(0.8))
            near = np.abs(t - np.rint(t)) <= F32(WRAP_EPS)
            dens = max(F32(density), F32(0.0))
            if dens > F32(0.01):
                angle = np.arctan2(ezy.astype(F32), ezx.astype(F32))
                mod = F32(0.5) + F32(0.5) * np.sin(angle * dens + smooth.astype(F32) * F32(0.25))
                t2 = t + F32(0.1) * mod
                near |= np.abs(t2 - np.rint(t2)) <= F32(WRAP_EPS)
        n += int((near & (t != F32(1.0))).sum())
    return n
