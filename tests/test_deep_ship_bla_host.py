"""Deep Burning Ship views with bilinear approximation (FR_FLAG_DEEP_SHIP_BLA): the parts that need no GPU -- the ABI, the
validation, the bound on |dc|, what the restatement (tests/deep_ship_bla_ref.py) skips and where it differs from the
unflagged one, and the structure of the ship's linear map the table's norm relies on."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

import deep_ship_bla_ref as SB
import deep_ship_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 256, 192
REAL_AXIS = dict(cx="-1.75", cy="0", zoom=1e-20, max_iter=500)       # Y = 0 throughout: every r is 0

# every (W, H, aa) a GPU test of the flag renders (test_deep_ship_bla_gpu.py, test_deep_ship_bla_footprint_gpu.py)
GPU_FRAMES = [(256, 192, 1), (256, 192, 2), (64, 48, 1), (64, 48, 2), (203, 117, 2), (160, 120, 1),
              (1, 1, 1), (7, 5, 1), (203, 117, 1)]
GPU_ZOOMS = [1.0, 3.0, 0.2, 1e-20, 1e-30, 1e-100, 2e-100]


@functools.lru_cache(maxsize=None)
def _orbit(name):
    v = S.VIEWS[name]
    return S.reference_orbit(v["cx"], v["cy"], v["zoom"], v["max_iter"])


@functools.lru_cache(maxsize=None)
def _flagged(name):
    """computed once per view, shared, never changed"""
    (planes,), counts = SB.restate_bla(S.VIEWS[name], W, H, orbit=_orbit(name))
    return planes, counts


@functools.lru_cache(maxsize=None)
def _unflagged(name):
    (planes,), _, _ = S.restate(S.VIEWS[name], W, H, orbit=_orbit(name))
    return planes


def test_flag_counts_and_table_are_in_the_header_and_capi(fr):
    hdr = open(os.path.join(ROOT, "include", "fractalrenderer_amd.h")).read()
    assert re.search(r"#define FR_FLAG_DEEP_SHIP_BLA\s+0x8u", hdr)
    assert re.search(r"#define FR_HAS_DEEP_SHIP_BLA 1", hdr)
    assert re.search(r"int fr_ctx_last_deep_ship_steps\(fr_ctx\* ctx, uint64_t out\[3\]\);", hdr)
    assert "Out of scope: BLA for the ship" not in hdr
    internal = open(os.path.join(ROOT, "fractalrenderer_amd", "csrc", "fr_internal.h")).read()
    assert re.search(r"int64_t fr_deep_ship_bla_table\(fr_ctx\* ctx, double\* r, double\* ab, int64_t n\);", internal)
    assert fr._capi.FR_FLAG_DEEP_SHIP_BLA == 0x8 == fr.FR_FLAG_DEEP_SHIP_BLA
    assert "FR_FLAG_DEEP_SHIP_BLA" in fr.__all__
    assert "fr_ctx_last_deep_ship_steps" in fr._capi.SIGNATURES
    assert "fr_deep_ship_bla_table" in fr._capi.INTERNAL_SIGNATURES
    assert hasattr(fr.lib(), "fr_ctx_last_deep_ship_steps") and hasattr(fr.lib(), "fr_deep_ship_bla_table")
    assert inspect.signature(fr.Renderer.render_deep_ship).parameters["bla"].default is False
    assert callable(fr.Renderer.last_deep_ship_steps)
    # the three flags are distinct bits next to the post chain's
    assert sorted((fr._capi.FR_FLAG_POST_CHAIN, fr.FR_FLAG_DEEP_BLA, fr.FR_FLAG_DEEPX_BLA, fr.FR_FLAG_DEEP_SHIP_BLA)) == [1, 2, 4, 8]


def test_the_ship_validator_accepts_its_own_flag_only(fr):
    F = fr._capi
    L = fr.lib()
    v = S.SHIP_A
    cv = fr.DeepView(v["cx"], v["cy"]).to_c()

    def check(flags):
        p = fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"]).to_params(fr.FractalType.BurningShip, fr.Precision.F64)
        p.flags = flags
        return L.fr_deep_ship_validate(C.byref(p), C.byref(cv), 64, 48)

    assert check(0) == F.FR_OK
    assert check(F.FR_FLAG_DEEP_SHIP_BLA) == F.FR_OK
    assert check(F.FR_FLAG_DEEP_SHIP_BLA | F.FR_FLAG_POST_CHAIN) == F.FR_OK
    assert check(F.FR_FLAG_DEEP_BLA) == F.FR_ERR_UNSUPPORTED
    assert check(F.FR_FLAG_DEEPX_BLA) == F.FR_ERR_UNSUPPORTED
    assert check(F.FR_FLAG_DEEP_SHIP_BLA | F.FR_FLAG_DEEP_BLA) == F.FR_ERR_UNSUPPORTED
    assert check(F.FR_FLAG_DEEP_SHIP_BLA | F.FR_FLAG_DEEPX_BLA) == F.FR_ERR_UNSUPPORTED


@pytest.mark.parametrize("geom", GPU_FRAMES, ids=lambda g: "%dx%d-aa%d" % g)
def test_every_sample_offset_is_below_dcmax(geom):
    """the table's radii assume |dc| < dcmax for every sub-sample of the frame, the ones outside [0, 1) included"""
    w, h, aa = geom
    for zoom in GPU_ZOOMS:
        bound = SB.dcmax(w, h, zoom)
        worst = 0.0
        for s in range(aa * aa):
            dcx, dcy = S.sample_dc(w, h, zoom, aa, s)
            worst = max(worst, float(np.sqrt(dcx * dcx + dcy * dcy).max()))
        assert worst < bound, (geom, zoom, worst, bound)
    # Mandelbrot's bound would not do: at aa 2 on a small frame the ship's offsets exceed its 1e-7 margin
    if (w, h, aa) == (64, 48, 2):
        import deep_bla_ref as BR
        dcx, dcy = S.sample_dc(w, h, 1.0, aa, 0)
        assert float(np.sqrt(dcx * dcx + dcy * dcy).max()) > BR.dcmax(w, h, 1.0)


@pytest.mark.parametrize("name,want", [("A", (4843014, 133801, 3624220)), ("B", (6736364, 195201, 20548362))])
def test_what_the_restatement_skips_is_pinned(name, want):
    """256 x 192, aa 1.  A: 42.8 % of the updates skipped, 1.70x fewer trips; B: 75.3 %, 3.94x"""
    v = S.VIEWS[name]
    (it, _), counts = _flagged(name)
    assert tuple(counts) == want
    updates = int(np.where(it < v["max_iter"], it.astype(np.int64) + 1, v["max_iter"]).sum())
    assert counts[0] + counts[2] == updates                          # every update is a plain step or skipped
    share = counts[2] / updates
    trips = updates / (counts[0] + counts[1])
    assert (round(share, 3), round(trips, 2)) == {"A": (0.428, 1.70), "B": (0.753, 3.94)}[name]


def test_no_bla_step_where_dc_is_large_or_the_orbit_is_real():
    for name in ("shallow", "needle"):
        (it, r2), counts = _flagged(name)
        pit, pr2 = _unflagged(name)
        assert counts[1] == 0 and counts[2] == 0, name
        assert np.array_equal(it, pit) and np.array_equal(r2.view(np.uint64), pr2.view(np.uint64)), name
    orb = S.reference_orbit(REAL_AXIS["cx"], REAL_AXIS["cy"], REAL_AXIS["zoom"], REAL_AXIS["max_iter"])
    assert len(orb) - 1 >= 3 and not orb[:, 1].any()
    tab = SB.bla_table(orb, SB.dcmax(64, 48, REAL_AXIS["zoom"]))
    assert len(tab) >= 1 and all(np.all(T["r"] == 0.0) for T in tab)
    samples, counts = SB.restate_bla(REAL_AXIS, 64, 48, 2, orbit=orb)
    plain, _, _ = S.restate(REAL_AXIS, 64, 48, 2, orbit=orb)
    assert counts[1] == 0 and counts[2] == 0
    for (it, r2), (pit, pr2) in zip(samples, plain):
        assert np.array_equal(it, pit) and np.array_equal(r2.view(np.uint64), pr2.view(np.uint64))


def test_flagged_and_unflagged_restatements_agree():
    """A: equal everywhere.  B: 23 of 49152 pixels differ (an escape inside a skipped stretch or a rounding away)"""
    (it, _), _ = _flagged("A")
    assert np.array_equal(it, _unflagged("A")[0])
    (it, _), _ = _flagged("B")
    differ = int((it != _unflagged("B")[0]).sum())
    assert differ == 23
    assert 1.0 - differ / it.size >= 0.999


def test_without_radius_it_is_the_plain_step():
    """eps = 0: every r is 0, no BLA step is taken and the planes are deep_ship_ref.perturb's, bit for bit"""
    (planes,), counts = SB.restate_bla(S.SHIP_A, 64, 48, orbit=_orbit("A"), eps=0.0)
    (plain,), _, _ = S.restate(S.SHIP_A, 64, 48, orbit=_orbit("A"))
    assert counts[1] == 0 and counts[2] == 0
    assert np.array_equal(planes[0], plain[0]) and np.array_equal(planes[1].view(np.uint64), plain[1].view(np.uint64))


@pytest.mark.parametrize("name", ["A", "B"])
def test_table_shape_and_monotone_radius(name):
    orb = _orbit(name)
    N = len(orb) - 1
    tab = SB.bla_table(orb, SB.dcmax(W, H, S.VIEWS[name]["zoom"]))
    assert len(tab) == (N - 1).bit_length() - 1
    assert sum(len(T["r"]) for T in tab) == (N - 1) - bin(N - 1).count("1")
    prev = SB.single_steps(orb)["r"]
    assert np.all(prev <= SB.EPS * np.sqrt(orb[1:N, 0] ** 2 + orb[1:N, 1] ** 2) * (1 + 2 ** -50))
    assert np.all(prev <= np.abs(orb[1:N, 0])) and np.all(prev <= np.abs(orb[1:N, 1]))      # the fold conditions
    for k, T in enumerate(tab, 1):
        assert len(T["r"]) == (N - 1) >> k
        assert np.all(T["r"] >= 0.0) and np.all(T["r"] <= prev[0:2 * len(T["r"]):2])
        prev = T["r"]
    assert any(np.any(T["r"] > 0.0) for T in tab)


@pytest.mark.parametrize("name", ["A", "B"])
def test_level_one_columns_have_equal_length(name):
    """A is 2 |Z_m| times a rotation or reflection, and so is a product of two: |A_x| as the first column's length is the
    operator norm.  Both columns of every level-1 A agree to within 4 ulp."""
    orb = _orbit(name)
    T = SB.bla_table(orb, SB.dcmax(W, H, S.VIEWS[name]["zoom"]))[0]
    c1 = np.sqrt(T["a11"] * T["a11"] + T["a21"] * T["a21"])
    c2 = np.sqrt(T["a12"] * T["a12"] + T["a22"] * T["a22"])
    assert np.all(np.abs(c1 - c2) <= 4.0 * np.spacing(np.maximum(c1, c2)))
    # and they are orthogonal to the same accuracy, relative to their lengths
    dot = T["a11"] * T["a12"] + T["a21"] * T["a22"]
    assert np.all(np.abs(dot) <= 8.0 * SB.EPS * c1 * c2)
