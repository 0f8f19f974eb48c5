"""The parameter cases of test_deep_cases_gpu.py as data, and the CPU predicates that say what each of them can see.

The deep-view kernels (fr_deep.hip.h: the sixteen instantiations of deep_kernel<ARGS> in KERNELS below) are tested elsewhere on many views and always with the FractalState defaults.  Here the views are few
and the parameters vary: everything the validators accept (fr_deep_validate, fr_deepx_validate, fr_deep_ship_validate,
fr_deepx_ship_validate, fr_deep_julia_validate, fr_deepx_julia_validate, fr_deep_de_validate) and the one host path
(DeepPath<BASE>, enqueue_deep_view, launch_deep in fr_device.hip) turns into a kernel's argument block, DeepBlock<F, X, DE, BLA>
-- a flagged kernel's is the base block with the table behind it.  Every one of the sixteen kernels runs in some case (test_deep_cases_host.py asserts it from PATHS).

A case is Case(path, view, params, W, H):
  path    a key of KERNELS: deep | ship | julia | de, an x for the extended arithmetic, _bla for the flagged kernel
  view    a key of VIEWS
  params  overrides of the FractalState defaults (FractalState's field names), "post": the post chain, and on the DE paths
          "shade" / "edge_px": the distance shading
  W, H    96 x 64 (twelve sub-tile columns, whole sub-tiles) or RAGGED, 100 x 37

GROUPS:
  bailout      2, 128 and 65536 on the deep views (B2 = 4: the smallest circle of the table log2; 2^32: r2 up to 2^65,
               de = |z| log|z| / |D| with |z| up to 2^32)
  small        bailout <= 1: lib_log, log_bailout of the eight ship and Julia blocks, the library log of values below 1
               (centres: below); on Julia a critical orbit Q of one or two updates and a flagged render with no table for Q
  short        reference orbits of N = 1, 2, 3 updates: the m == N rebase on every trip, K = 0 and the one-entry table; on
               Julia the primary orbit P is the short one
  max_iter     max_iterations 1, 2, 3 through every loop form; on Julia a frame with samples escaping at every update
  colour       every palette mode, colour scale / offset, interior style, brightness / saturation / contrast; the same
               under the distance shading
  aa           antialiasing_samples 3 and 4 on a ragged frame with the post chain
  ship_noop    stripe_enabled without interior style 2: accepted by fr_deep_ship_validate, read by nothing
  julia_noop   interior styles, orbit trap, stripes: accepted by fr_deep_julia_validate, read by nothing

The predicates work on the restatements only (test_deep_cases_host.py::test_cases_can_fail asserts them for every case);
whether a GPU comparison means anything is decided there, on the CPU, never by the GPU test about itself.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import deep_bla_ref as BR
import deep_de_ref as DE
import deep_julia_bla_ref as JB
import deep_julia_ref as J
import deep_ref as R
import deep_ship_bla_ref as SB
import deep_ship_ref as S
import deepx_bla_ref as XB
import deepx_de_ref as XD
import deepx_ref as X
import deepx_ship_bla_ref as XSB
import deepx_ship_ref as XS
from cases import JULIA_PALETTES, MANDEL_PALETTES

Case = namedtuple("Case", "path view params W H")
# samples: per sub-sample (iter, r2); counts: the three step counts of a flagged path; N: the updates of the reference
# orbit (Julia: of P); D: per sub-sample (Dx, Dy) or (Dx, Dy, eD) on the DE paths; NQ: the updates of Julia's critical
# orbit; stats: what the restatement counted beside (Julia: rebases, bla_p, bla_q)
Restated = namedtuple("Restated", "samples counts N D NQ stats", defaults=(None, None, None))

W0, H0 = 96, 64
RAGGED = (100, 37)
# path -> the kernel instantiation it launches, as fr_device.hip names it in messages (deep_kernel_name: the switches of the
# path's DeepBlock<F, X, DE, BLA> that are on)
_SWITCHES = {"deep": "Mandel", "deepx": "Mandel, X", "ship": "Ship", "shipx": "Ship, X", "julia": "Julia", "juliax": "Julia, X",
             "de": "Mandel, DE", "dex": "Mandel, X, DE"}
KERNELS = {p + b: "deep_kernel<%s%s>" % (s, ", BLA" if b else "") for p, s in _SWITCHES.items() for b in ("", "_bla")}
PATHS = tuple(KERNELS)
OLD_PATHS = ("deep", "deep_bla", "deepx", "deepx_bla", "ship")     # the paths of the table before the other eleven
SHIP_PATHS = ("ship", "ship_bla", "shipx", "shipx_bla")
JULIA_PATHS = ("julia", "julia_bla", "juliax", "juliax_bla")
DE_PATHS = ("de", "de_bla", "dex", "dex_bla")
EXTENDED = ("deepx", "deepx_bla", "shipx", "shipx_bla", "dex", "dex_bla")      # the view's zoom is a string
FLAGGED = tuple(p for p in PATHS if p.endswith("_bla"))


def formula(path) -> int:
    """the oracle's fractal number of the path's colour stage: 0 Mandelbrot, 1 Julia, 2 Burning Ship"""
    return 2 if path in SHIP_PATHS else 1 if path in JULIA_PATHS else 0


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

# ---- Julia views -------------------------------------------------------------------------------------------------------
# deep_julia_ref's views centred on the fixed point alpha of z^2 + c, and shallow views with a short PRIMARY orbit P: the
# centre lies outside the filled Julia set, P ends after N_P updates (|P_N| > 4), every sample that survives them leaves
# P at m == N_P and follows the critical orbit Q from then on.  Measured on deep_julia_ref.restate at 96 x 64:
#
#   view   c               centre    zoom  max_iter  N_P  surviving  rebases  bar (0.9 surviving max_iter / N_P)
#   J_N1   (0, 1)          (2.5, 0)  6     3         1    6.6 %      1802     1091
#   J_N2   (-0.12, 0.74)   (1.5, 0)  4     24        2    5.5 %      4396     3640
#   J_N3   (-0.12, 0.74)   (1.2, 0)  3     32        3    9.7 %      6296     5750
#
# max_iter is the largest of 3, 4, 8, 12, 16, 24, 32, 48, 64 at which the frame passes test_cases_can_fail.  The dendrite
# (c = i) has no interior: 4.5 % survive four updates and nothing survives 64, so J_N1 stops at 3, as M_N1 stops at 2;
# c = i at (1.6, 0), zoom 4 has N_P = 2 and the same fate (2.8 % at max_iter 8), so N_P = 2 runs on the rabbit.  The rabbit's
# interior falls onto its attracting 3-cycle, where a delta shrinks and no longer rebases: at max_iter 48 the rebases of
# J_N2 / J_N3 are 4460 / 6322 against bars of 7106 / 8568.  (From there on the flagged restatement takes BLA steps on Q --
# 233 / 420 at max_iter 48 -- which these frames therefore do not have; Q's table is walked by RABBIT30: 35 720 steps.)
# J_N3's one-entry table of P (N_P = 3) takes exactly one step in the frame.
def _julia(c, cx, cy, zoom, max_iter):
    """a shallow Julia view in deep_julia_ref's form: F is what the library chooses for the zoom"""
    return dict(c=c, cx=cx, cy=cy, zoom=zoom, zoom_s=repr(zoom), max_iter=max_iter, F=R.frac_bits(zoom))


J_N1 = _julia((0.0, 1.0), "2.5", "0", 6.0, 3)
J_N2 = _julia((-0.12, 0.74), "1.5", "0", 4.0, 24)
J_N3 = _julia((-0.12, 0.74), "1.2", "0", 3.0, 32)
SHORT_N = {"M_N1": 1, "M_N2": 2, "M_N3": 3, "S_N1": 1, "S_N2": 2, "S_N3": 3, "J_N1": 1, "J_N2": 2, "J_N3": 3}
# At max_iterations 1, 2, 3 the frame of J_N3 splits into 2, 3 and 4 iter classes (N_P = 1, 2, 3: the centre's own orbit is
# cut by max_iterations as well); at 3 they hold 2233 / 1397 / 781 / 1733 samples.

# RABBIT30 (c = -0.12 + 0.74i, 1e-30, max_iter 1100): 30.5 % escape at bailouts 2, 4 and 65536, between updates 709 and 731.
# With |c| = 0.7497 its critical orbit has N_Q = 2 at bailout 0.75 (N_P = 1061), and 32.6 % of the samples leave P for it;
# DENDRITE30 (c = i) has N_Q = 1 there and no sample leaves P, N_Q = 2 at bailout 1 (37.3 % leave); DUST30 (c = -0.8 +
# 0.156i) has N_Q = 1 at bailout 0.75 and 4.0 % of its samples walk it: every update of theirs is a rebase.
# DUST30C is DUST30 with max_iter 1200 for 1600: of DUST30's samples 98.4 % escape (updates 1076 .. 1600), of RABBIT30's
# 30.5 %, of DENDRITE30's all -- outside the 0.50 .. 0.90 of the colour cases; at 1200 80 % of DUST30's do.
VIEWS = {"A": R.VIEW_A, "SHIP_A": S.SHIP_A, "D": X.views()["D"],
         "SMALL_M": SMALL_M, "SMALL_S": SMALL_S, "UNIT_M": UNIT_M, "UNIT_S": UNIT_S,
         "M_N1": M_N1, "M_N2": M_N2, "M_N3": M_N3, "S_N1": S_N1, "S_N2": S_N2, "S_N3": S_N3,
         # extended views: deepx_ship_ref's ship at 1e-310 (72 % escape, 73 classes; its TIP400 escapes whole, in 8 classes, and
         # the average of a pixel's sub-samples is sample 0's colour there), deepx_ref's T130 (starts extended, turns plain)
         "S310": XS.views()["S310"], "T130": X.views()["T130"],
         "RABBIT30": J.view("RABBIT30"), "DENDRITE30": J.view("DENDRITE30"), "DUST30": J.view("DUST30"),
         "DUST30C": dict(J.view("DUST30"), max_iter=1200),
         "J_N1": J_N1, "J_N2": J_N2, "J_N3": J_N3}

BAILOUTS = (2.0, 128.0, 65536.0)
SCALE_OFFSET = ((0.37, 0.21), (3.0, -0.4), (0.0, 0.5))
# SHIP_A escapes late (nu / max_iter in [0.74, 1], half of it below 0.76) and the ship's palettes saturate above 0.8: with
# (3.0, -0.4) the bulk lands on fract(1.82 .. 1.88), saturated like the default plane, and 0.24 of the pixels differ from
# it -- short of the 0.25 of test_cases_can_fail.  The ship runs the neighbouring (3.0, -0.2) instead: fract(2.02 .. 2.08).
SCALE_OFFSET_SHIP = ((0.37, 0.21), (3.0, -0.2), (0.0, 0.5))
BSC = dict(color_brightness=1.3, color_saturation=0.6, color_contrast=1.2)
# Under BSC the post chain saturates every escaped pixel of A and D (0.9054924 in all three channels), shaded or not: a
# dropped shading passes there.  The shaded cases turn the brightness down instead, and the shading stays visible.
BSC_SHADED = dict(BSC, color_brightness=0.7)
INTERIOR = {"deep": (0, 1, 3), "deepx": (0, 1, 3), "ship": (0, 1, 2), "julia": (),      # what each validator accepts
            "dex_bla": (0, 1, 3), "de": (0, 1, 3)}                                     # (Julia's styles: julia_noop)
COLOUR_VIEWS = (("deep", "A"), ("ship", "SHIP_A"), ("deepx", "D"), ("julia", "DUST30C"), ("dex_bla", "D"))
SHADED_VIEWS = (("dex_bla", "D"), ("de", "A"))           # the colour cases again under the distance shading
SHADE = dict(shade=True, edge_px=1.8)
X_SHIP = "S310"                                          # the extended ship view of the bailout and max_iter cases
# what each Julia small case is there for beside the bailout: N_Q as measured above
SMALL_NQ = {("RABBIT30", 0.75): 2, ("DENDRITE30", 0.75): 1, ("DENDRITE30", 1.0): 2, ("DUST30", 0.75): 1}
JULIA_NOOP = (dict(interior_style=1), dict(interior_style=2), dict(interior_style=3), dict(orbit_trap_enabled=True),
              dict(stripe_enabled=True))


def _case(path, view, W=W0, H=H0, **params):
    return Case(path, view, params, W, H)


def _palettes(path):
    return MANDEL_PALETTES if formula(path) == 0 else JULIA_PALETTES          # as test_all_palettes enumerates them


def _scale_offset(path):
    return SCALE_OFFSET_SHIP if formula(path) == 2 else SCALE_OFFSET          # (DUST30C passes the bar with Mandelbrot's pairs)


def _groups():
    g = {k: {} for k in ("bailout", "small", "short", "max_iter", "colour", "aa", "ship_noop", "julia_noop")}
    for b in BAILOUTS:
        for path, view in (("deep", "A"), ("deep_bla", "A"), ("ship", "SHIP_A"), ("deepx", "D")):
            g["bailout"][f"{path}-{view}-b{b:g}"] = _case(path, view, bailout=b)
    g["bailout"]["deepx_bla-D-b65536"] = _case("deepx_bla", "D", bailout=65536.0)
    for b in BAILOUTS:
        for path, view in (("ship_bla", "SHIP_A"), ("shipx", X_SHIP), ("shipx_bla", X_SHIP), ("julia", "RABBIT30"),
                           ("julia_bla", "RABBIT30"), ("juliax", "RABBIT30"), ("juliax_bla", "RABBIT30"), ("de", "A"),
                           ("de_bla", "A"), ("dex", "D"), ("dex_bla", "D")):
            g["bailout"][f"{path}-{view}-b{b:g}"] = _case(path, view, bailout=b)
    for path, view, b in (("deep", "SMALL_M", 0.75), ("ship", "SMALL_S", 0.75), ("deep", "UNIT_M", 0.75),
                          ("ship", "UNIT_S", 0.75), ("deep", "UNIT_M", 1.0), ("ship", "UNIT_S", 1.0)):
        g["small"][f"{path}-{view}-b{b:g}"] = _case(path, view, bailout=b)
    for path in JULIA_PATHS:
        for view, b in (("RABBIT30", 0.75), ("DENDRITE30", 0.75), ("DUST30", 0.75), ("RABBIT30", 1.0), ("DENDRITE30", 1.0)):
            g["small"][f"{path}-{view}-b{b:g}"] = _case(path, view, bailout=b)
    for path in ("ship_bla", "shipx", "shipx_bla"):
        for view, b in (("SMALL_S", 0.75), ("UNIT_S", 0.75), ("UNIT_S", 1.0)):
            g["small"][f"{path}-{view}-b{b:g}"] = _case(path, view, bailout=b)
    for view, b in (("SMALL_M", 0.75), ("UNIT_M", 0.75), ("UNIT_M", 1.0)):
        g["small"][f"dex-{view}-b{b:g}"] = _case("dex", view, bailout=b)
    for n in (1, 2, 3):
        for path in ("deep", "deep_bla"):
            g["short"][f"{path}-M_N{n}"] = _case(path, f"M_N{n}")
        g["short"][f"ship-S_N{n}"] = _case("ship", f"S_N{n}")
    for n in (1, 3):
        for path in ("deepx", "deepx_bla"):
            g["short"][f"{path}-M_N{n}"] = _case(path, f"M_N{n}")
    for n in (1, 2, 3):
        for path in JULIA_PATHS:
            g["short"][f"{path}-J_N{n}"] = _case(path, f"J_N{n}")
        for path in ("ship_bla", "shipx"):
            g["short"][f"{path}-S_N{n}"] = _case(path, f"S_N{n}")
    for mi in (1, 2, 3):
        for path, view in (("deep", "A"), ("deep_bla", "A"), ("ship", "SHIP_A"), ("deepx_bla", "D")):
            g["max_iter"][f"{path}-{view}-mi{mi}"] = _case(path, view, max_iterations=mi)
    for mi in (1, 2, 3):
        for path, view in (("ship_bla", "SHIP_A"), ("shipx_bla", X_SHIP), ("dex_bla", "D"), ("de", "A")):
            g["max_iter"][f"{path}-{view}-mi{mi}"] = _case(path, view, max_iterations=mi)
        for path in JULIA_PATHS:
            g["max_iter"][f"{path}-J_N3-mi{mi}"] = _case(path, "J_N3", max_iterations=mi)
    for path, view in COLOUR_VIEWS:
        for m in _palettes(path):
            g["colour"][f"{path}-palette{m}"] = _case(path, view, palette_mode=m)
        for sc, off in _scale_offset(path):
            g["colour"][f"{path}-scale{sc:g}-offset{off:g}"] = _case(path, view, color_scale=sc, color_offset=off)
        for st in INTERIOR[path]:
            g["colour"][f"{path}-interior{st}"] = _case(path, view, interior_style=st)
        g["colour"][f"{path}-bsc"] = _case(path, view, post=True, **BSC)
    for path, view in SHADED_VIEWS:
        for m in _palettes(path):
            g["colour"][f"{path}-shaded-palette{m}"] = _case(path, view, palette_mode=m, **SHADE)
        for sc, off in _scale_offset(path):
            g["colour"][f"{path}-shaded-scale{sc:g}-offset{off:g}"] = _case(path, view, color_scale=sc, color_offset=off, **SHADE)
        for st in INTERIOR[path]:
            g["colour"][f"{path}-shaded-interior{st}"] = _case(path, view, interior_style=st, **SHADE)
        g["colour"][f"{path}-shaded-bsc"] = _case(path, view, post=True, **BSC_SHADED, **SHADE)
    for aa in (3, 4):
        for path, view in (("deep", "A"), ("ship", "SHIP_A")):
            g["aa"][f"{path}-{view}-aa{aa}"] = _case(path, view, *RAGGED, antialiasing_samples=aa, post=True)
    for aa in (3, 4):
        for path, view in (("julia", "DUST30C"), ("juliax_bla", "DUST30C"), ("shipx", X_SHIP)):
            g["aa"][f"{path}-{view}-aa{aa}"] = _case(path, view, *RAGGED, antialiasing_samples=aa, post=True)
        g["aa"][f"dex-T130-shaded-aa{aa}"] = _case("dex", "T130", *RAGGED, antialiasing_samples=aa, post=True, **SHADE)
    for st in (0, 1):
        g["ship_noop"][f"ship-stripes-interior{st}"] = _case("ship", "SHIP_A", stripe_enabled=True, interior_style=st)
    for q in JULIA_NOOP:
        (k, v), = q.items()
        g["julia_noop"][f"julia-{k}{int(v)}"] = _case("julia", "DUST30C", **q)
    return g


GROUPS = _groups()
CASES = {f"{group}/{name}": case for group, cases in GROUPS.items() for name, case in cases.items()}
GROUP_OF = {f"{group}/{name}": group for group, cases in GROUPS.items() for name in cases}
GROUPS_BY_ID = {group: [f"{group}/{name}" for name in cases] for group, cases in GROUPS.items()}


# ---- a case on the CPU -------------------------------------------------------------------------------------------------
def view_of(case) -> dict:
    """the view with the case's max_iterations; the zoom a double or, on the EXTENDED paths, a string.  A Julia view holds
    both (zoom and zoom_s, as deep_julia_ref's) with c and F, and serves all four Julia paths as it is."""
    v = dict(VIEWS[case.view])
    v["max_iter"] = int(case.params.get("max_iterations", v["max_iter"]))
    assert ("c" in v) == (case.path in JULIA_PATHS), "a Julia view is for the Julia paths, and no other is"
    if "c" in v:
        return v
    extended = case.path in EXTENDED
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
    counts = D = NQ = stats = None
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
    elif path == "ship_bla":
        orbit = S.reference_orbit(v["cx"], v["cy"], v["zoom"], max_iter, bailout)
        (samples, counts), N = SB.restate_bla(v, W, H, aa, bailout, orbit=orbit), len(orbit) - 1
    elif path == "shipx":
        orbit = XS.orbit_of(v, bailout)
        samples, N = XS.restate_ship_x(v, W, H, aa, bailout, orbit=orbit), len(orbit[1]) - 1
    elif path == "shipx_bla":
        orbit = XS.orbit_of(v, bailout)
        (samples, counts), N = XSB.restate_ship_x_bla(v, W, H, aa, bailout, orbit=orbit), len(orbit[1]) - 1
    elif path in ("julia", "julia_bla"):
        P, Q = J.reference_orbits(v, bailout)
        N, NQ, stats = len(P) - 1, len(Q) - 1, {}
        if path == "julia":
            samples = J.restate(v, W, H, aa, bailout, orbits=(P, Q), stats=stats)
        else:
            samples, counts = JB.restate_bla(v, W, H, aa, bailout, orbits=(P, Q), stats=stats)
    elif path in ("juliax", "juliax_bla"):
        Px, Qx = J.reference_orbits_x(v, bailout)
        N, NQ, stats = len(Px[1]) - 1, len(Qx[1]) - 1, {}
        if path == "juliax":
            samples = J.restate_x(v, W, H, aa, bailout, orbits=(Px, Qx), stats=stats)
        else:
            samples, counts = JB.restate_x_bla(v, W, H, aa, bailout, orbits=(Px, Qx), stats=stats)
    elif path in ("de", "de_bla"):
        orbit = R.reference_orbit(v["cx"], v["cy"], v["zoom"], max_iter, bailout)
        (full, counts), N = DE.restate_de(v, W, H, aa, bailout, orbit=orbit, bla=path == "de_bla"), len(orbit) - 1
        samples, D = [s[:2] for s in full], [s[2:] for s in full]
    elif path in ("dex", "dex_bla"):
        orbit = X.orbit_of(v, bailout)
        (full, counts), N = XD.restate_x_de(v, W, H, aa, bla=path == "dex_bla", bailout=bailout, orbit=orbit), len(orbit[1]) - 1
        samples, D = [s[:2] for s in full], [s[2:] for s in full]
    else:
        raise ValueError(path)
    if path not in FLAGGED:
        counts = None                                            # the DE restatements count the plain steps of an empty table
    for planes in list(samples) + list(D or ()):
        for a in planes:
            a.setflags(write=False)
    return Restated(tuple(tuple(s) for s in samples), None if counts is None else tuple(int(c) for c in counts), N,
                    None if D is None else tuple(tuple(d) for d in D), NQ, stats)


def restated(case) -> Restated:
    return _restate(case.path, case.view, view_of(case)["max_iter"], bailout_of(case), aa_of(case), case.W, case.H)


@functools.lru_cache(maxsize=None)
def rebases(ship: bool, view, max_iter, bailout, W, H) -> int:
    """the rebases of the plain step over the frame (a property of the view: the BLA and extended paths share it)"""
    v = dict(VIEWS[view], max_iter=max_iter)
    return (S if ship else R).restate(v, W, H, 1, bailout)[1]


def rebases_of(case) -> int:
    """rebases() of the case's view; Julia's from the stats of the unflagged fp64 restatement of the same frame"""
    max_iter = view_of(case)["max_iter"]
    if case.path in JULIA_PATHS:
        return _restate("julia", case.view, max_iter, bailout_of(case), 1, case.W, case.H).stats["rebases"]
    return rebases(case.path in SHIP_PATHS, case.view, max_iter, bailout_of(case), case.W, case.H)


def smooth(case, it, r2) -> np.ndarray:
    """nu of the path's shader: Mandelbrot's, or the form the ship and Julia share"""
    v = view_of(case)
    return (R if formula(case.path) == 0 else S).smooth(it, r2, v["max_iter"], bailout_of(case))


def expected_nu(case) -> np.ndarray:
    return smooth(case, *restated(case).samples[0])


def de_of(case, s: int = 0) -> np.ndarray:
    """the distance estimate of sub-sample s of a DE path"""
    r, max_iter = restated(case), view_of(case)["max_iter"]
    return (XD.de_of_x if case.path in EXTENDED else DE.de_of)(*r.samples[s], *r.D[s], max_iter)


def expected_de(case) -> np.ndarray:
    return de_of(case, 0)


def expected_deriv(case) -> np.ndarray:
    """the deriv plane of a DE path: D of sample 0's escaping update, zeros for interior"""
    r, max_iter = restated(case), view_of(case)["max_iter"]
    return (XD.deriv_of_x if case.path in EXTENDED else DE.deriv_of)(r.samples[0][0], *r.D[0], max_iter)


COLOUR_KEYS = ("palette_mode", "color_scale", "color_offset", "interior_style", "color_brightness", "color_saturation",
               "color_contrast")


def expected_rgb(oracle, case, params=None) -> np.ndarray:
    """The oracle's colour stage on the restated samples, as the _expected_rgba helpers of the deep GPU tests build it:
    per-sample colour in the fp64 path of the shader (Mandelbrot's, Julia's or the Burning Ship's), on a DE path with
    "shade" the distance shading of every escaped sub-sample (deep_de_ref.shade, as test_deep_de_gpu._expected_shaded), the
    supersample average in the order of `samples` (the shader's: sy outer for Mandelbrot, sx outer for the ship and Julia
    -- the order matters through the float summation only), then the post chain (the ship's and Julia's with Julia's
    floors).  `params` replaces the case's colour parameters (the default plane of a predicate, a deliberately wrong
    build)."""
    q = case.params if params is None else params
    v = view_of(case)
    f = formula(case.path)
    aa = aa_of(case)
    p = oracle.OracleParams(fractal=f, max_iterations=v["max_iter"], zoom=1.0, aa=aa, post_chain=0,
                            palette_mode=int(q.get("palette_mode", 0)), color_scale=float(q.get("color_scale", 1.0)),
                            color_offset=float(q.get("color_offset", 0.0)), interior_style=int(q.get("interior_style", 0)))
    shade = bool(q.get("shade", False))
    assert not shade or case.path in DE_PATHS
    acc = np.zeros((case.H, case.W, 3), np.float32)
    for s, (it, r2) in enumerate(restated(case).samples):
        rgb = oracle.colorize(p, smooth(case, it, r2))[..., :3]
        if shade:
            rgb = DE.shade(rgb, de_of(case, s), it < v["max_iter"], float(q["edge_px"]))
        acc = acc + rgb
    if aa > 1:
        acc = acc / np.float32(aa * aa)
    if q.get("post", False):
        b, s, c = (float(q.get(k, 1.0)) for k in ("color_brightness", "color_saturation", "color_contrast"))
        acc = np.array([oracle.post_chain(px, b, s, c, julia_floors=int(f != 0)) for px in acc.reshape(-1, 3)],
                       np.float32).reshape(case.H, case.W, 3)
    return acc


def default_params(case) -> dict:
    """the case's parameters with every colour parameter at its default; the post chain and the shading stay as the case
    has them"""
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
# are black under every accepted style).  Julia's palette table is the ship's: modes 0 .. 9.  A "same" case cannot fail by the kernel ignoring the parameter; it fails when
# the kernel acts on it, which is what a table lookup past the defined modes or a style test written != 0 would do.
def colour_expectation(case) -> str:
    q = case.params
    mandel = formula(case.path) == 0
    if "palette_mode" in q:
        defined = range(1, 6) if mandel else range(1, 10)
        return "differs" if q["palette_mode"] in defined else "same"
    if "interior_style" in q:
        return "interior" if (mandel and q["interior_style"] == 1) else "same"
    return "differs"
