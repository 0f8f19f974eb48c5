"""Views whose lanes fall back from the plain mode to the extended one (tests/deepx_return_ref.py): the parts that need no GPU.
Conditions on the references alone that keep the views honest -- how often a lane returns, how many escape classes a frame
has --, the recordings of tests/golden/deepx_return.npz against fresh computations, the restatement against the exact
iteration on every recorded pixel, the library's reference orbit against Python integers, and the proof that the views see the
plain-to-extended block: the restatement with that block's arithmetic changed no longer gives the exact frame."""
import numpy as np
import pytest

import deep_julia_ref as J
import deep_ref as R
import deepx_phoenix_ref as PX
import deepx_ref as X
import deepx_return_ref as RET
import deepx_ship_ref as SX

W, H = RET.SIZE
V = RET.views()
ROWS_320 = [0, 8, 17]


@pytest.fixture(scope="module")
def fresh130():
    """deepx_ref.restate_x of the whole RET130 frame: ((iter, r2), stats), computed once, never changed"""
    st = {}
    return X.restate_x(V["RET130"], W, H, stats=st)[0], st


# ---- the views are what they are meant to be: conditions on the references alone ---------------------------------------------
def test_views_are_one_centre_at_two_depths():
    a, b = V["RET130"], V["RET320"]
    assert (a["cx"], a["cy"]) == (b["cx"], b["cy"]) and len(a["cx"].lstrip("-0.")) == 400 == len(a["cy"].lstrip("-0."))
    assert a["cx"].startswith("-0.1010963638456221610257853922205719158211209466065984966648507")
    assert a["cy"].startswith("0.95628651080914150077109604531786904665245438804261290019135219")
    assert (a["zoom"], a["max_iter"], b["zoom"], b["max_iter"]) == ("1e-130", 50000, "1e-320", 152000)
    assert X.frac_bits_x(b["zoom"]) == 1216 and float(b["zoom"]) < 1e-290 <= float(a["zoom"])


@pytest.mark.parametrize("name,per_lane", [("RET130", 20), ("RET320", 40)])
def test_lanes_return_to_the_extended_mode_many_times(name, per_lane):
    """measured at 24 x 18: 11522 returns on RET130 (26.7 per lane), 28625 on RET320 (66.3 per lane)"""
    st = RET.stats(name)
    print(name, st, "to_ext per lane", st["to_ext"] / (W * H))
    assert st["to_ext"] >= per_lane * W * H
    assert st["to_plain"] >= st["to_ext"]
    if name == "RET130":
        assert st["plain_steps"] > st["ext_steps"] > 0
    else:
        assert st["ext_steps"] > st["plain_steps"] > 0


@pytest.mark.parametrize("name", RET.NAMES)
def test_frames_have_many_escape_classes(name):
    """at least 100 distinct escape indices and no class above 5 % of the pixels.  RET130: of the exact frame.  RET320 has exact
    values on 64 pixels only, so the conditions are on the restated frame, which equals the exact values wherever they are recorded
    (test_restated_iter_is_the_exact_iteration_on_every_recorded_pixel)"""
    mi = V[name]["max_iter"]
    it = RET.exact(name) if name == "RET130" else RET.golden(name, "iter").ravel()
    assert it.size == W * H
    vals, cnt = np.unique(it[it < mi], return_counts=True)
    print(name, "distinct", len(vals), "range", vals[0], vals[-1], "largest class", cnt.max(), "interior", int((it == mi).sum()))
    assert len(vals) >= 100
    assert max(cnt.max(), int((it == mi).sum())) <= 0.05 * it.size


# ---- the recordings ---------------------------------------------------------------------------------------------------------------
def test_recorded_restatement_of_ret130_is_a_fresh_one(fresh130):
    (it, r2), st = fresh130
    assert np.array_equal(it, RET.golden("RET130", "iter"))
    assert np.array_equal(r2.view(np.uint64), RET.golden("RET130", "r2").view(np.uint64))
    assert st == RET.stats("RET130")


def test_recorded_restatement_of_ret320_is_a_fresh_one_on_three_rows():
    it, r2 = X.restate_x(V["RET320"], W, H, rows=ROWS_320)[0]
    assert np.array_equal(it, RET.golden("RET320", "iter")[ROWS_320])
    assert np.array_equal(r2.view(np.uint64), RET.golden("RET320", "r2")[ROWS_320].view(np.uint64))


@pytest.mark.parametrize("name", RET.NAMES)
def test_recorded_exact_values_are_the_exact_iteration(name):
    """the four corners and one more pixel, Mandelbrot's exact iteration and Phoenix's at p = r = 0 (its bailout is 2)"""
    ys, xs = RET.exact_pixels(name)
    ex, pex = RET.exact(name), RET.exact(name, phoenix=True)
    assert len(ys) == len(ex) == len(pex) == (W * H if name == "RET130" else 64)
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    picked = [int(np.flatnonzero((ys == y) & (xs == x))[0]) for y, x in corners] + [len(ex) // 2 + 5]
    assert len(set((int(ys[k]), int(xs[k])) for k in picked)) == 5
    pv = dict(V[name], p=0.0, r=0.0)
    for k in picked:
        x, y = int(xs[k]), int(ys[k])
        assert X.exact_iter_x(V[name], x, y, W, H) == ex[k], (x, y)
        assert PX.exact_iter_x(pv, x, y, W, H) == pex[k], (x, y)


@pytest.mark.parametrize("name", RET.NAMES)
def test_restated_iter_is_the_exact_iteration_on_every_recorded_pixel(name):
    """equality on every pixel, for each of the five restatements: plain, BLA, the two DE forms, and Phoenix at p = r = 0 against
    its own exact values"""
    ys, xs = RET.exact_pixels(name)
    ex = RET.exact(name)
    for key in ("iter", "bla_iter", "de_iter", "debla_iter"):
        it = RET.golden(name, key)
        assert it.shape == (H, W) and it.dtype == np.int32
        assert np.array_equal(it[ys, xs], ex), (key, int((it[ys, xs] != ex).sum()))
    assert np.array_equal(RET.golden(name, "px_iter")[ys, xs], RET.exact(name, phoenix=True))
    counts = RET.golden(name, "bla_counts")
    assert counts[1] > 0 and counts[2] > counts[0] and np.array_equal(counts, RET.golden(name, "debla_counts"))
    if name == "RET130":
        assert tuple(counts) == (120465, 140917, 19213710)


@pytest.mark.parametrize("name", RET.NAMES)
def test_library_orbit_is_the_python_integer_orbit(fr, name):
    """the orbit returns to about 1 / 1.35e25 once per period of 201: far above the double range, every exponent 0"""
    v = V[name]
    mant, exp2 = fr.deepx_reference_orbit(fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"]), v["max_iter"])
    pm, pe = X.orbit_of(v)
    assert len(pe) == v["max_iter"] + 1                              # the centre never escapes
    assert np.array_equal(mant.view(np.uint64), pm.view(np.uint64)) and np.array_equal(exp2, pe)
    assert pe[0] == X.X_ZERO and not pe[1:].any()
    back = np.abs(pm[201:2011:201]).max(axis=1)
    assert np.all(back < 1e-24) and np.all(back > 1e-27)


# ---- the views see the plain-to-extended block ------------------------------------------------------------------------------------
def test_fp64_restatement_of_ret130_is_the_extended_one_bit_for_bit(fresh130):
    """deep_ref.restate knows no extended mode: an independent statement of what the returns must give"""
    v = V["RET130"]
    (it, r2), _ = fresh130
    (pit, pr2), = R.restate(dict(v, zoom=float(v["zoom"])), W, H)[0]
    assert np.array_equal(pit.reshape(H, W), it)
    assert np.array_equal(pr2.reshape(H, W).view(np.uint64), r2.view(np.uint64))


def _plus_one(x, y, e, norm):
    bx, by, be = norm(x, y, e)
    return bx, by, be + 1


def _exponent_not_set(x, y, e, norm):
    bx, by, _ = norm(x, y, e)
    return bx, by, e


@pytest.mark.parametrize("change", [_plus_one, _exponent_not_set], ids=["be+1", "exponent-not-set"])
def test_restatement_with_a_changed_return_path_misses_the_exact_frame(monkeypatch, change):
    """perturb_x normalises with exponent 0 in one place only, the plain step's return to the extended mode (every other call
    passes the zoom's or a delta's exponent, all below -400): changing the arithmetic of that call alone, the restated RET130 frame
    differs from the exact one on more than half the pixels.  (Leaving dz as it is, with exponent 0, is no such change: it is
    the same number, no product of the following steps leaves the double range at this depth, and the frame comes out the same.)"""
    norm = X._norm
    hits = []

    def patched(x, y, e):
        if e.size and not e.any():
            hits.append(e.size)
            return change(x, y, e, norm)
        return norm(x, y, e)

    monkeypatch.setattr(X, "_norm", patched)
    it = X.restate_x(V["RET130"], W, H)[0][0]
    ndiff = int((it.ravel() != RET.exact("RET130")).sum())
    print(change.__name__, "pixels that differ from the exact frame", ndiff, "of", it.size)
    assert hits
    assert ndiff > it.size // 2


# ---- the coverage the other families have -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S310", "S400"])
def test_ship_views_return_on_a_quarter_of_the_lanes(name):
    """measured at 24 x 18: S310 144 returns, S400 278 (0.33 and 0.64 per lane); the BLA ship tests render the same two views"""
    st = {}
    SX.restate_ship_x(SX.views()[name], W, H, stats=st)
    print(name, st)
    assert st["to_ext"] >= 0.25 * W * H


def test_phoenix_view_with_r_returns_on_half_of_the_lanes():
    """PXRET, r = -0.5: measured 367 returns on 432 lanes"""
    st = {}
    PX.restate_x(PX.PXRET, W, H, stats=st)
    print("PXRET", st)
    assert PX.PXRET["r"] != 0.0 and st["to_ext"] >= 0.5 * W * H


@pytest.mark.parametrize("name", ["DENDRITE400", "DENDRITE1000"])
def test_julia_views_count_their_mode_changes(name):
    """Neither extended Julia view returns a lane to the extended mode (to_ext 0 at 24 x 18 and at 48 x 36), nor does DENDRITE400's
    centre at the zooms {1, 2, 4, 7}e-{125, 200, 300, 350, 400}: the reference is a fixed point, dz grows until the rebase, and
    the critical orbit of a dendrite never comes back to 0.  So no floor is set for Julia; what is pinned is that the count exists and that
    every lane but the centre's leaves the extended mode once."""
    _, st = J.restated_x(name, 1, W, H)
    print(name, st)
    assert "to_ext" in st and st["to_plain"] == W * H - 1
