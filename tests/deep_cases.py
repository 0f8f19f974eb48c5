"""The parameter cases of test_deep_cases_gpu.py as data, and the CPU predicates that say what each of them can see.

The deep-view kernels (fr_deep.hip.h: the eight instantiations deep_kernel<Deep[Ship][X][Bla]Args> -- DeepArgs, DeepBlaArgs,
DeepXArgs, DeepXBlaArgs, DeepShipArgs, DeepShipBlaArgs, DeepShipXArgs, DeepShipXBlaArgs) are tested elsewhere on many
views and always with the FractalState defaults.  Here the views are few and the parameters vary: everything
fr_deep_validate, fr_deepx_validate and fr_deep_ship_validate accept and fill_deep_args (fr_device.hip) turns into kernel
arguments by hand.  The cases run the five paths below (the first five of the eight kernels); the other three ship kernels
read the same argument block through the same colour stage.

A case is Case(path, view, params, W, H):
  path    deep | deep_bla | deepx | deepx_bla | ship
  view    a key of VIEWS
  params  overrides of the FractalState defaults (FractalState's field names) and "post": the post chain
  W, H    96 x 64 (twelve sub-tile columns, whole sub-tiles) or RAGGED, 100 x 37

GROUPS:
  bailout      2, 128 and 65536 on the deep views (B2 = 4: the smallest circle of the table log2; 2^32: r2 up to 2^65)
  small        bailout <= 1: lib_log, DeepShipArgs::log_bailout, the library log of values below 1 (centres: below)
  short        reference orbits of N = 1, 2, 3 updates: the m == N rebase on every trip, K = 0 and the one-entry table
  max_iter     max_iterations 1, 2, 3 through every loop form
  colour       every palette mode, colour scale / offset, interior style, brightness / saturation / contrast
  aa           antialiasing_samples 3 and 4 on a ragged frame with the post chain
  ship_noop    stripe_enabled without interior style 2: accepted by fr_deep_ship_validate, read by nothing

The predicates work on the restatements only (test_deep_cases_host.py::test_cases_can_fail asserts them for every case);
whether a GPU comparison means anything is decided there, on the CPU, never by the GPU test about itself.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import deep_bla_ref as BR
import deep_ref as R
import deep_ship_ref as S
import deepx_bla_ref as XB
import deepx_ref as X
from cases import JULIA_PALETTES, MANDEL_PALETTES

Case = namedtuple("Case", "path view params W H")
Restated = namedtuple("Restated", "samples counts N")

W0, H0 = 96, 64
RAGGED = (100, 37)
PATHS = ("deep", "deep_bla", "deepx", "deepx_bla", "ship")
RGB_TOL = 1e-4                        # test_deep_gpu.RGB_TOL (asserted equal in test_deep_cases_gpu.py)

# ---- the centres of the bailout <= 1 cases ---------------------------------------------------------------------------
# How they were found (mpmath, 90 digits, on the host).  With bailout b <= 1 a sample escapes at the first update k with
# |z_k(c)| > b, so a frame has more than one iter class only where a level curve |z_k(c)| = b crosses it.  A coarse scan
# of the parameter plane (1400 x 1400, 300 updates) gave the cells in which the largest |z_k| of a bounded orbit is about
# 0.75 and is reached at a late update, next to a cell where it is reached at another update; from there Newton's method
# in (Re c, Im c) on the two equations |z_k1(c)|^2 = b1^2, |z_k2(c)|^2 = b2^2 (Jacobian by differences of 1e-45), to
# 1e-70.  For the ship the scan kept the orbits that stay in one quadrant, so that no fold changes branch near the centre.
#
#   SMALL_M  inside the main cardioid: |z_18| = |z_20| = 0.75, every other |z_k| <= 0.7414 (600 updates)
#   SMALL_S  inside the ship's main body, orbit in the fourth quadrant: |z_19| = |z_21| = 0.75, every other <= 0.7353
#   UNIT_M   beside the cusp of the cardioid (outside the set): |z_7| = 0.75, |z_9| = 1, |z_k| increasing
#   UNIT_S   the same construction for the ship, orbit in the first quadrant: |z_9| = 0.75, |z_11| = 1
#
# SMALL_*: at bailout 0.75 two level curves cross at the centre: samples escape at update k1, at update k2, or never.
# At bailout 1 exactly nothing escapes there (no |z_k| exceeds 0.75), so the bailout = 1 cases -- lib_log is
# !(bailout > 1) -- run on UNIT_*, where a level curve of |z_k| = 1 crosses the frame as well: r2 of the samples that
# escape on it is 1 + a few 1e-11, where log(r2) is all relative precision and the table log2 of the other branch
# (absolute error 1e-16) would be wrong in the sixth digit of nu.
#
# The zoom is 1e-12, not deeper: the escape test reads r2 of z = Z_m + dz in double, so a level curve is resolved only
# while dz is not absorbed by Z_m (|dz| ~ 100 zoom against ulp(0.75) = 1e-16).  At 1e-30 both the kernel and the
# restatement give one class for the whole frame and agree with the exact iteration on half of it.  The frames are
# offset from the crossing by (0.071, 0.043) view heights, as views A and B are from their Misiurewicz point.
_SMALL_M0 = ("-0.7260683664658440867402200902337643337892674", "0.1498883668973762753699316691235646972292854")
_SMALL_S0 = ("0.3807818457725917315227421526901687012584243", "-0.6029197850408093286777023139532635632706583")
_UNIT_M0 = ("0.3112872145937561934200379156298264302145119", "0.0202309818531411462243127504560905379878641")
_UNIT_S0 = ("0.2936634256498367522640661863452290473359380", "0.0081034656463126654483862082768172027276004")
SMALL_ZOOM = 1e-12


def _offset(c0, zoom):
    """the crossing less (0.071, 0.043) view heights, as exact decimal strings"""
    from decimal import Decimal, getcontext
    getcontext().prec = 80
    z = Decimal(repr(zoom))
    return dict(cx=str(Decimal(c0[0]) - Decimal("0.071") * z), cy=str(Decimal(c0[1]) - Decimal("0.043") * z))


SMALL_M = dict(_offset(_SMALL_M0, SMALL_ZOOM), zoom=SMALL_ZOOM, max_iter=64)
SMALL_S = dict(_offset(_SMALL_S0, SMALL_ZOOM), zoom=SMALL_ZOOM, max_iter=64)
UNIT_M = dict(_offset(_UNIT_M0, SMALL_ZOOM), zoom=SMALL_ZOOM, max_iter=64)
UNIT_S = dict(_offset(_UNIT_S0, SMALL_ZOOM), zoom=SMALL_ZOOM, max_iter=64)

# ---- short reference orbits --------------------------------------------------------------------------------------------
# Shallow views whose centre lies outside the set: the reference orbit ends after N updates (|Z_N| > 4), the frame still
# holds the set.  Found by hand from the recurrence: Mandelbrot 5 -> 25 + 5; 1.57 -> 4.03 -> ..; 1.2 -> 2.64 -> 8.17 -> ..;
# the ship's with deep_ship_ref.reference_orbit.  max_iter is the largest at which at least 0.05 of the samples survive
# (test_cases_can_fail): with N = 1 the centre is further than 4 from the origin, the frame is wide and the set is 0.75 %
# of it, so max_iter is 2 there -- two updates, both rebased, both prefetches clamped.
M_N1 = dict(cx="5", cy="0", zoom=12.0, max_iter=2)
M_N2 = dict(cx="1.57", cy="0", zoom=4.5, max_iter=256)
M_N3 = dict(cx="1.2", cy="0", zoom=3.0, max_iter=256)
S_N1 = dict(cx="5", cy="0", zoom=12.0, max_iter=2)
S_N2 = dict(cx="1.6", cy="-0.5", zoom=4.5, max_iter=64)
S_N3 = dict(cx="1.3", cy="-0.5", zoom=4.0, max_iter=256)
SHORT_N = {"M_N1": 1, "M_N2": 2, "M_N3": 3, "S_N1": 1, "S_N2": 2, "S_N3": 3}

VIEWS = {"A": R.VIEW_A, "SHIP_A": S.SHIP_A, "D": X.views()["D"],
         "SMALL_M": SMALL_M, "SMALL_S": SMALL_S, "UNIT_M": UNIT_M, "UNIT_S": UNIT_S,
         "M_N1": M_N1, "M_N2": M_N2, "M_N3": M_N3, "S_N1": S_N1, "S_N2": S_N2, "S_N3": S_N3}

BAILOUTS = (2.0, 128.0, 65536.0)
SCALE_OFFSET = ((0.37, 0.21), (3.0, -0.4), (0.0, 0.5))
# SHIP_A escapes late (nu / max_iter in [0.74, 1], half of it below 0.76) and the ship's palettes saturate above 0.8: with
# (3.0, -0.4) the bulk lands on fract(1.82 .. 1.88), saturated like the default plane, and 0.24 of the pixels differ from
# it -- short of the 0.25 of test_cases_can_fail.  The ship runs the neighbouring (3.0, -0.2) instead: fract(2.02 .. 2.08).
SCALE_OFFSET_SHIP = ((0.37, 0.21), (3.0, -0.2), (0.0, 0.5))
BSC = dict(color_brightness=1.3, color_saturation=0.6, color_contrast=1.2)
INTERIOR = {"deep": (0, 1, 3), "deepx": (0, 1, 3), "ship": (0, 1, 2)}      # what each validator accepts
COLOUR_VIEWS = (("deep", "A"), ("ship", "SHIP_A"), ("deepx", "D"))


def _case(path, view, W=W0, H=H0, **params):
    return Case(path, view, params, W, H)


def _groups():
    g = {k: {} for k in ("bailout", "small", "short", "max_iter", "colour", "aa", "ship_noop")}
    for b in BAILOUTS:
        for path, view in (("deep", "A"), ("deep_bla", "A"), ("ship", "SHIP_A"), ("deepx", "D")):
            g["bailout"][f"{path}-{view}-b{b:g}"] = _case(path, view, bailout=b)
    g["bailout"]["deepx_bla-D-b65536"] = _case("deepx_bla", "D", bailout=65536.0)
    for path, view, b in (("deep", "SMALL_M", 0.75), ("ship", "SMALL_S", 0.75), ("deep", "UNIT_M", 0.75),
                          ("ship", "UNIT_S", 0.75), ("deep", "UNIT_M", 1.0), ("ship", "UNIT_S", 1.0)):
        g["small"][f"{path}-{view}-b{b:g}"] = _case(path, view, bailout=b)
    for n in (1, 2, 3):
        for path in ("deep", "deep_bla"):
            g["short"][f"{path}-M_N{n}"] = _case(path, f"M_N{n}")
        g["short"][f"ship-S_N{n}"] = _case("ship", f"S_N{n}")
    for n in (1, 3):
        for path in ("deepx", "deepx_bla"):
            g["short"][f"{path}-M_N{n}"] = _case(path, f"M_N{n}")
    for mi in (1, 2, 3):
        for path, view in (("deep", "A"), ("deep_bla", "A"), ("ship", "SHIP_A"), ("deepx_bla", "D")):
            g["max_iter"][f"{path}-{view}-mi{mi}"] = _case(path, view, max_iterations=mi)
    for path, view in COLOUR_VIEWS:
        for m in (JULIA_PALETTES if path == "ship" else MANDEL_PALETTES):      # as test_all_palettes enumerates them
            g["colour"][f"{path}-palette{m}"] = _case(path, view, palette_mode=m)
        for sc, off in (SCALE_OFFSET_SHIP if path == "ship" else SCALE_OFFSET):
            g["colour"][f"{path}-scale{sc:g}-offset{off:g}"] = _case(path, view, color_scale=sc, color_offset=off)
        for st in INTERIOR[path]:
            g["colour"][f"{path}-interior{st}"] = _case(path, view, interior_style=st)
        g["colour"][f"{path}-bsc"] = _case(path, view, post=True, **BSC)
    for aa in (3, 4):
        for path, view in (("deep", "A"), ("ship", "SHIP_A")):
            g["aa"][f"{path}-{view}-aa{aa}"] = _case(path, view, *RAGGED, antialiasing_samples=aa, post=True)
    for st in (0, 1):
        g["ship_noop"][f"ship-stripes-interior{st}"] = _case("ship", "SHIP_A", stripe_enabled=True, interior_style=st)
    return g


GROUPS = _groups()
CASES = {f"{group}/{name}": case for group, cases in GROUPS.items() for name, case in cases.items()}
GROUP_OF = {f"{group}/{name}": group for group, cases in GROUPS.items() for name in cases}
GROUPS_BY_ID = {group: [f"{group}/{name}" for name in cases] for group, cases in GROUPS.items()}


# ---- a case on the CPU -------------------------------------------------------------------------------------------------
def view_of(case) -> dict:
    """the view with the case's max_iterations; the zoom a double (deep, deep_bla, ship) or a string (deepx, deepx_bla)"""
    v = dict(VIEWS[case.view])
    v["max_iter"] = int(case.params.get("max_iterations", v["max_iter"]))
    extended = case.path in ("deepx", "deepx_bla")
    if extended and not isinstance(v["zoom"], str):
        v["zoom"] = repr(v["zoom"])
    assert extended or not isinstance(v["zoom"], str), "a view below the double range needs an extended path"
    return v


def bailout_of(case) -> float:
    return float(case.params.get("bailout", 4.0))


def aa_of(case) -> int:
    return int(case.params.get("antialiasing_samples", 1))


@functools.lru_cache(maxsize=None)
def _restate(path, view, max_iter, bailout, aa, W, H):
    """computed once per (path, view, max_iter, bailout, aa, frame), shared by every case and test, read-only"""
    v = view_of(Case(path, view, dict(max_iterations=max_iter), W, H))
    counts = None
    if path == "deep":
        orbit = R.reference_orbit(v["cx"], v["cy"], v["zoom"], max_iter, bailout)
        samples, N = R.restate(v, W, H, aa, bailout, orbit=orbit)[0], len(orbit) - 1
    elif path == "deep_bla":
        orbit = R.reference_orbit(v["cx"], v["cy"], v["zoom"], max_iter, bailout)
        (samples, counts), N = BR.restate_bla(v, W, H, aa, bailout, orbit=orbit), len(orbit) - 1
    elif path == "ship":
        orbit = S.reference_orbit(v["cx"], v["cy"], v["zoom"], max_iter, bailout)
        samples, N = S.restate(v, W, H, aa, bailout, orbit=orbit)[0], len(orbit) - 1
    elif path == "deepx":
        orbit = X.orbit_of(v, bailout)
        samples, N = X.restate_x(v, W, H, aa, bailout, orbit=orbit), len(orbit[1]) - 1
    elif path == "deepx_bla":
        orbit = X.orbit_of(v, bailout)
        (samples, counts), N = XB.restate_x_bla(v, W, H, aa, bailout, orbit=orbit), len(orbit[1]) - 1
    else:
        raise ValueError(path)
    for it, r2 in samples:
        it.setflags(write=False); r2.setflags(write=False)
    return Restated(tuple(samples), None if counts is None else tuple(int(c) for c in counts), N)


def restated(case) -> Restated:
    return _restate(case.path, case.view, view_of(case)["max_iter"], bailout_of(case), aa_of(case), case.W, case.H)


@functools.lru_cache(maxsize=None)
def rebases(ship: bool, view, max_iter, bailout, W, H) -> int:
    """the rebases of the plain step over the frame (a property of the view: the BLA and extended paths share it)"""
    v = dict(VIEWS[view], max_iter=max_iter)
    return (S if ship else R).restate(v, W, H, 1, bailout)[1]


def smooth(case, it, r2) -> np.ndarray:
    v = view_of(case)
    return (S if case.path == "ship" else R).smooth(it, r2, v["max_iter"], bailout_of(case))


def expected_nu(case) -> np.ndarray:
    return smooth(case, *restated(case).samples[0])


COLOUR_KEYS = ("palette_mode", "color_scale", "color_offset", "interior_style", "color_brightness", "color_saturation",
               "color_contrast")


def expected_rgb(oracle, case, params=None) -> np.ndarray:
    """The oracle's colour stage on the restated samples, as the _expected_rgba helpers of the deep GPU tests build it:
    per-sample colour in the fp64 path of the shader (Mandelbrot's or the Burning Ship's), the supersample average in the
    order of `samples` (the shader's: sy outer for Mandelbrot, sx outer for the ship -- the order matters through the float
    summation only), then the post chain (the ship's with Julia's floors).  `params` replaces the case's colour parameters
    (the default plane of a predicate, a deliberately wrong build)."""
    q = case.params if params is None else params
    v = view_of(case)
    ship = case.path == "ship"
    aa = aa_of(case)
    p = oracle.OracleParams(fractal=2 if ship else 0, max_iterations=v["max_iter"], zoom=1.0, aa=aa, post_chain=0,
                            palette_mode=int(q.get("palette_mode", 0)), color_scale=float(q.get("color_scale", 1.0)),
                            color_offset=float(q.get("color_offset", 0.0)), interior_style=int(q.get("interior_style", 0)))
    acc = np.zeros((case.H, case.W, 3), np.float32)
    for it, r2 in restated(case).samples:
        acc = acc + oracle.colorize(p, smooth(case, it, r2))[..., :3]
    if aa > 1:
        acc = acc / np.float32(aa * aa)
    if q.get("post", False):
        b, s, c = (float(q.get(k, 1.0)) for k in ("color_brightness", "color_saturation", "color_contrast"))
        acc = np.array([oracle.post_chain(px, b, s, c, julia_floors=int(ship)) for px in acc.reshape(-1, 3)],
                       np.float32).reshape(case.H, case.W, 3)
    return acc


def default_params(case) -> dict:
    """the case's parameters with every colour parameter at its default; the post chain stays as the case has it"""
    return {k: v for k, v in case.params.items() if k not in COLOUR_KEYS}


def differing(a, b, tol=10 * RGB_TOL) -> np.ndarray:
    """mask of the pixels whose colours differ by more than tol in some channel (a NaN on one side only differs)"""
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) > tol
    return (d | (np.isnan(a) != np.isnan(b))).any(axis=2)


# what the shader makes of a colour case, beside the default plane: "differs" (the 0.25 predicate), "interior" (interior
# style 1 of Mandelbrot blackens the interior samples and nothing else) or "same" -- a value the shader maps onto the
# default (palette modes outside the defined ones fall back to mode 0's palette; interior styles 1 and 2 of the ship
# need the orbit trap or the stripes, style 3 of Mandelbrot does not exist in its shader; interior samples of the ship
# are black under every accepted style).  A "same" case cannot fail by the kernel ignoring the parameter; it fails when
# the kernel acts on it, which is what a table lookup past the defined modes or a style test written != 0 would do.
def colour_expectation(case) -> str:
    q = case.params
    ship = case.path == "ship"
    if "palette_mode" in q:
        defined = range(1, 10) if ship else range(1, 6)
        return "differs" if q["palette_mode"] in defined else "same"
    if "interior_style" in q:
        return "interior" if (not ship and q["interior_style"] == 1) else "same"
    return "differs"
