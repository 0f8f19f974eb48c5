"""Deep Burning Ship views with extended-exponent deltas (fr_render_deepx_ship): the parts that need no GPU -- the header
macros and exported symbols, the reference orbit in the extended storage against Python integers, validation, the
restatement's fold against exact rationals, the restatement against deep_ship_ref's on views a double holds, and
fr_deep_sequence_plan unchanged by the ship sequences."""
import ctypes as C
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import deep_ship_ref as S
import deepx_ref as X
import deepx_ship_ref as SX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = SX.views()


def _view(fr, cx="-1.75", cy="-0.03", zoom="1e-400", frac_bits=0, reserved=0):
    enc = lambda s: s.encode() if isinstance(s, str) else s
    return fr._capi.fr_deepx_view(enc(cx), enc(cy), enc(zoom), frac_bits, reserved)


def _orbit(fr, v, max_iter, bailout=4.0):
    mant = np.empty((max_iter + 1, 2), np.float64)
    exp2 = np.empty(max_iter + 1, np.int32)
    n = C.c_int32()
    st = fr.lib().fr_deepx_ship_reference_orbit(C.byref(v), max_iter, C.c_float(bailout), mant.ctypes.data, exp2.ctypes.data,
                                                C.byref(n))
    return st if st else (mant[:n.value].copy(), exp2[:n.value].copy())


# ---- ABI -----------------------------------------------------------------------------------------------------------
def test_header_macros_and_symbols(fr, tmp_path):
    for name in ("fr_deepx_ship_reference_orbit", "fr_render_deepx_ship", "fr_render_deepx_ship_async",
                 "fr_deep_ship_sequence_create"):
        assert name in fr._capi.SIGNATURES and getattr(fr.lib(), name)
    assert callable(fr.deepx_ship_reference_orbit) and callable(fr.Renderer.render_deepx_ship)
    gcc = shutil.which("gcc")
    if gcc:
        src = tmp_path / "macros.c"
        src.write_text("#include \"fractalrenderer_amd.h\"\n"
                       "#if !defined(FR_HAS_DEEPX_SHIP) || FR_HAS_DEEPX_SHIP != 1\n#error FR_HAS_DEEPX_SHIP\n#endif\n"
                       "#if !defined(FR_HAS_DEEP_SHIP_SEQUENCE) || FR_HAS_DEEP_SHIP_SEQUENCE != 1\n#error FR_HAS_DEEP_SHIP_SEQUENCE\n#endif\n"
                       "int (*a)(const fr_deepx_view*, int32_t, float, double*, int32_t*, int32_t*) = fr_deepx_ship_reference_orbit;\n"
                       "int (*b)(fr_ctx*, const fr_params*, const fr_deepx_view*, uint32_t, uint32_t, const fr_shard*, const fr_output*)"
                       " = fr_render_deepx_ship;\n"
                       "int (*c)(fr_ctx*, const fr_params*, const fr_deepx_view*, uint32_t, uint32_t, const fr_shard*, const fr_output*,"
                       " void*) = fr_render_deepx_ship_async;\n"
                       "int (*d)(fr_ctx*, const fr_params*, const fr_deep_sequence_desc*, uint32_t, uint32_t, fr_deep_sequence**)"
                       " = fr_deep_ship_sequence_create;\n")
        subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "macros.o")], check=True)


# ---- the reference orbit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S400", "TIP1000", "NUC546"])
def test_orbit_matches_python_integers_in_the_extended_storage(fr, name):
    v = V[name]
    n = v["max_iter"]                                              # the whole orbit the view runs with
    F = X.frac_bits_x(v["zoom"])
    mant, exp2 = SX.reference_orbit_x_ship(v["cx"], v["cy"], F, n)
    got = _orbit(fr, _view(fr, v["cx"], v["cy"], v["zoom"]), n)
    assert np.array_equal(got[0].view(np.uint64), mant.view(np.uint64)) and np.array_equal(got[1], exp2)
    m2, e2 = fr.deepx_ship_reference_orbit(fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"]), n)
    assert np.array_equal(m2.view(np.uint64), mant.view(np.uint64)) and np.array_equal(e2, exp2)
    assert exp2[0] == X.X_ZERO
    if name == "NUC546":                                           # the orbit returns far below the double range
        assert len(exp2) == n + 1 and exp2[546] < -1100 and 0.5 <= np.abs(mant[546]).max() < 1.0
    if name == "TIP1000":                                          # the real axis: Y = 0 exactly, points signed
        assert np.all(mant[:, 1] == 0.0) and mant[1, 0] == -2.0 and mant[2, 0] == 2.0
    # the plain doubles are those of fr_deep_ship_reference_orbit at the same F wherever a double holds the point
    old = np.empty((n + 1, 2)); ln = C.c_int32()
    dv = fr._capi.fr_deep_view(v["cx"].encode(), v["cy"].encode(), F, 0)
    assert fr.lib().fr_deep_ship_reference_orbit(C.byref(dv), 1e-100, n, C.c_float(4.0), old.ctypes.data, C.byref(ln)) == 0
    assert ln.value == len(exp2)
    normal = exp2 == 0
    assert np.array_equal(mant[normal].view(np.uint64), old[:ln.value][normal].view(np.uint64))


def test_shallow_views_get_the_orbit_of_fr_render_deep_ship(fr):
    for name in ("A", "B", "needle"):
        v = S.VIEWS[name]
        mant, exp2 = _orbit(fr, _view(fr, v["cx"], v["cy"], repr(v["zoom"])), v["max_iter"])
        want = S.reference_orbit(v["cx"], v["cy"], v["zoom"], v["max_iter"])
        assert np.array_equal(X.decode(mant, exp2).view(np.uint64), want.view(np.uint64)), name


# ---- validation ---------------------------------------------------------------------------------------------------------
def test_validation_with_no_device(fr):
    L, K = fr.lib(), fr._capi
    E, U = K.FR_ERR_INVALID_ARG, K.FR_ERR_UNSUPPORTED
    ship, f64 = fr.FractalType.BurningShip, fr.Precision.F64

    def check(p, v, w=8, h=8):
        return L.fr_deepx_ship_validate(C.byref(p), C.byref(v), w, h)

    ok = fr.FractalState(max_iterations=64).to_params(ship, f64, False)
    assert check(ok, _view(fr)) == 0
    big = fr.FractalState(max_iterations=64, zoom=1e30, center_x=1e30).to_params(ship, f64, False)
    assert check(big, _view(fr)) == 0                              # p->zoom and the double centre are ignored
    for flag in (K.FR_FLAG_DEEP_BLA, K.FR_FLAG_DEEPX_BLA, K.FR_FLAG_DEEP_SHIP_BLA):
        p = fr.FractalState(max_iterations=64).to_params(ship, f64, False)
        p.flags |= flag
        assert check(p, _view(fr)) == U, flag
    assert check(fr.FractalState(max_iterations=64).to_params(fr.FractalType.Mandelbrot, f64, False), _view(fr)) == U
    assert check(fr.FractalState(max_iterations=64).to_params(ship, fr.Precision.F32, False), _view(fr)) == U
    assert check(fr.FractalState(max_iterations=64, orbit_trap_enabled=True).to_params(ship, f64, False), _view(fr)) == U
    assert check(fr.FractalState(max_iterations=64, interior_style=3).to_params(ship, f64, False), _view(fr)) == U
    assert check(fr.FractalState(max_iterations=64, stripe_enabled=True, interior_style=2).to_params(ship, f64, False),
                 _view(fr)) == U
    assert check(fr.FractalState(max_iterations=64, stripe_enabled=True).to_params(ship, f64, False), _view(fr)) == 0
    assert check(fr.FractalState(max_iterations=64, bailout=1e6).to_params(ship, f64, False), _view(fr)) == E
    for z in ("1e-1001", "2e3", "z", "", "0", "-1"):
        assert check(ok, _view(fr, zoom=z)) == E, z
    assert check(ok, _view(fr, zoom="1e-1000")) == 0 and check(ok, _view(fr, zoom="1e3")) == 0
    assert check(ok, _view(fr, frac_bits=100)) == E and check(ok, _view(fr, reserved=1)) == E
    assert check(ok, _view(fr, cx="1e")) == E and check(ok, _view(fr, cy=None)) == E and check(ok, _view(fr, zoom=None)) == E
    assert L.fr_deepx_ship_validate(None, C.byref(_view(fr)), 8, 8) == E
    # the orbit entry: its own argument checks
    mant = np.empty((9, 2)); exp2 = np.empty(9, np.int32); n = C.c_int32()
    v = _view(fr)
    orbit = L.fr_deepx_ship_reference_orbit
    assert orbit(C.byref(v), 8, C.c_float(4.0), mant.ctypes.data, exp2.ctypes.data, C.byref(n)) == 0 and n.value >= 2
    assert orbit(C.byref(v), 0, C.c_float(4.0), mant.ctypes.data, exp2.ctypes.data, C.byref(n)) == E
    assert orbit(C.byref(v), 8, C.c_float(0.0), mant.ctypes.data, exp2.ctypes.data, C.byref(n)) == E
    assert orbit(C.byref(v), 8, C.c_float(4.0), None, exp2.ctypes.data, C.byref(n)) == E
    assert orbit(None, 8, C.c_float(4.0), mant.ctypes.data, exp2.ctypes.data, C.byref(n)) == E
    # the render entries check their arguments before they touch a device: ctx NULL comes first
    o = K.fr_output(None, None, None, K.FR_MEM_HOST, 0)
    assert L.fr_render_deepx_ship(None, C.byref(ok), C.byref(v), 8, 8, None, C.byref(o)) == E
    assert L.fr_render_deepx_ship_async(None, C.byref(ok), C.byref(v), 8, 8, None, C.byref(o), None) == E
    h = C.c_void_p()
    d = K.fr_deep_sequence_desc(b"-2", b"0", b"1e-310", b"2.5e-311", 5, 0, 0, 0)
    assert L.fr_deep_ship_sequence_create(None, C.byref(ok), C.byref(d), 8, 8, C.byref(h)) == E


def test_python_wrappers_reject_what_the_issue_names(fr):
    with pytest.raises(ValueError):
        fr.Renderer.render_deepx_ship(None, fr.FractalState(), 8, 8, fr.DeepView("-2", "0"))
    with pytest.raises(ValueError):
        fr.Renderer.render_deep_ship(None, fr.FractalState(), 8, 8, fr.DeepView("-2", "0", zoom="1e-400"))
    with pytest.raises(ValueError):
        fr.DeepZoomSequence(None, fr.FractalState(), "-2", "0", "1e-310", "2.5e-311", 5, 8, 8, formula="ship", xbla=True)
    with pytest.raises(ValueError):
        fr.DeepZoomSequence(None, fr.FractalState(), "-2", "0", "1e-310", "2.5e-311", 5, 8, 8, formula="julia")


# ---- the fold ------------------------------------------------------------------------------------------------------------
def test_fold_against_exact_rationals():
    """random (X, eZ, a, ed) with exponent gaps eZ - ed from -1100 to +1100: the fold in the delta's frame is
    |X 2^eZ + a 2^ed| - |X 2^eZ| in units of 2^ed to one rounding, flipped or not"""
    rng = np.random.default_rng(11)
    n = 4000
    gap = np.concatenate([rng.integers(-1100, 1101, n // 2), rng.integers(-3, 4, n // 2)])
    ed = rng.integers(-3300, -400, n)
    eZ = ed + gap
    Xm = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n)
    a = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n)
    Xm[:8] = 0.0                                                   # an orbit coordinate that is exactly 0: |a|
    with np.errstate(over="ignore"):                               # ldexp of a coordinate far above the delta: +-inf
        got, flip = SX.fold_x(Xm, eZ.astype(np.int64), a, ed.astype(np.int64))
    assert flip.sum() >= 200 and (~flip).sum() >= 200
    worst = {False: Fraction(0), True: Fraction(0)}
    for k in range(n):
        want = SX.fold_x_exact(float(Xm[k]), int(eZ[k]), float(a[k]), int(ed[k]))
        assert np.isfinite(got[k])
        err = abs(Fraction(float(got[k])) - want)
        if want != 0:
            rel = err / abs(want)
            worst[bool(flip[k])] = max(worst[bool(flip[k])], rel)
            assert rel <= Fraction(1, 1 << 52), (k, Xm[k], eZ[k], a[k], ed[k], float(rel))
        else:
            assert err == 0
    print("worst relative error: unflipped", float(worst[False]), "flipped", float(worst[True]))
    assert np.array_equal(got[:8], np.abs(a[:8]))
    # X far below the delta and of the other sign than a flips: the result is -(2 X 2^(eZ - ed) + a), |a| to one rounding
    far = (gap < -60) & (Xm != 0.0)
    assert np.array_equal(flip[far], (np.sign(Xm[far]) != np.sign(a[far])))
    # X far above the delta never flips, whatever ldexp overflows to
    assert not flip[(gap > 60) & (Xm != 0.0)].any()
    with np.errstate(over="ignore"):
        big, fl = SX.fold_x(np.array([0.75, -0.75]), np.array([0, 0], np.int64), np.array([0.5, 0.5]),
                            np.array([X.X_ZERO + 5, X.X_ZERO + 5], np.int64))
    assert np.array_equal(big, [0.5, -0.5]) and not fl.any()


# ---- the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,aa", [("A", 1), ("A", 2), ("B", 1), ("B", 2)])
def test_restatement_equals_deep_ship_refs_on_views_a_double_holds(name, aa):
    """dc >= 2^-400: every sample leaves the extended mode on its first step, (iter, r2) bit for bit those of
    deep_ship_ref.restate"""
    Wt, Ht = 64, 48
    v = S.VIEWS[name]
    stats = {}
    got = SX.restate_ship_x(SX.as_x_view(v), Wt, Ht, aa, stats=stats)
    want = S.restate(v, Wt, Ht, aa)[0]
    for (gi, gr), (wi, wr) in zip(got, want):
        assert np.array_equal(gi, wi) and np.array_equal(gr.view(np.uint64), wr.view(np.uint64)), name
    assert stats["to_ext"] == 0 and stats["ext_steps"] <= Wt * Ht * aa * aa + v["max_iter"], stats


@pytest.mark.parametrize("name", ["S310", "S400"])
def test_restatement_agrees_with_the_exact_iteration(name):
    g = SX.exact_golden()
    v, ex = V[name], g[name]
    stats = {}
    it = SX.restate_ship_x(v, 128, 96, pixels=(g["ys"], g["xs"]), stats=stats)[0][0]
    print(name, "agreement", (it == ex).mean(), stats)
    assert np.unique(ex, return_counts=True)[1].max() <= 0.60 * len(ex)
    assert (ex < v["max_iter"]).mean() >= 0.10
    assert (it == ex).mean() >= 0.99
    assert stats["ext_steps"] > stats["plain_steps"] and stats["to_plain"] > 0
    for k in (0, 97):                                              # the fixture is what exact_iter_ship_x gives
        assert SX.exact_iter_ship_x(v, int(g["xs"][k]), int(g["ys"][k]), 128, 96) == ex[k], k


def test_the_tipy300_frame_pins_the_2x_term_of_the_flipped_branch():
    """TIPY300's Y is stored nonzero (2^-1000 below X) and of the size of the deltas: extended folds flip on it, and a fold
    whose flipped branch forms d = X + a in place of 2X + a gives another iter plane on the frame the GPU test compares.
    The views whose flips all meet X = 0 (TIP400) cannot tell the two folds apart."""
    v = V["TIPY300"]
    mant, exp2 = SX.orbit_of(v)
    assert np.all(exp2[1:] == 0) and np.all(mant[1:, 1] != 0.0) and 0.0 < abs(mant[1, 1]) < 2.0 ** -990 * abs(mant[1, 0])
    stats = {}
    right = SX.restate_ship_x(v, 48, 36, orbit=(mant, exp2), stats=stats)[0][0]
    wrong = SX.restate_ship_x(v, 48, 36, orbit=(mant, exp2), fold=SX.fold_x_undoubled)[0][0]
    changed = int((right != wrong).sum())
    print(stats, "distinct", len(np.unique(right)), "iter changed by the wrong fold", changed)
    assert stats["flipped_ext"] >= 400 and stats["ext_steps"] > stats["plain_steps"] and stats["to_plain"] > 0
    assert len(np.unique(right)) >= 8 and changed >= 100
    rng = np.random.default_rng(5)                                 # the generator's samples: the right fold is the exact one
    ys, xs = rng.integers(0, 36, 40), rng.integers(0, 48, 40)
    ex = np.array([SX.exact_iter_ship_x(v, int(x), int(y), 48, 36) for x, y in zip(xs[:12], ys[:12])])
    assert np.array_equal(right[ys[:12], xs[:12]], ex)
    t = V["TIP400"]
    assert np.array_equal(SX.restate_ship_x(t, 48, 36)[0][0], SX.restate_ship_x(t, 48, 36, fold=SX.fold_x_undoubled)[0][0])


# ---- sequences ---------------------------------------------------------------------------------------------------------------
def test_sequence_plan_is_unchanged(fr):
    """fr_deep_sequence_plan knows no formula: the ship sequences share the descriptor, the walk and F"""
    import deep_seq_ref as Q
    L, K = fr.lib(), fr._capi
    v = V["S310"]
    for mode in (0, 1):
        d = K.fr_deep_sequence_desc(v["cx"].encode(), v["cy"].encode(), b"1e-310", b"2.5e-311", 5, 0, mode, 0)
        for f in range(5):
            out = K.fr_deep_sequence_frame()
            assert L.fr_deep_sequence_plan(C.byref(d), f, C.byref(out)) == 0
            want = Q.plan("1e-310", "2.5e-311", 5, f, mode)
            assert (out.zoom_mant, out.zoom_exp2, out.keyframe, out.resampled, out.u) == \
                (want["zoom_mant"], want["zoom_exp2"], want["keyframe"], want["resampled"], want["u"]), (mode, f)
            assert out.frac_bits == Q.auto_frac_bits("1e-310", "2.5e-311")
        assert L.fr_deep_sequence_plan(C.byref(d), 2, C.byref(out)) == 0
        assert (out.zoom_mant, out.zoom_exp2) == X.zoom_pair("5e-311") and out.keyframe == 1 and not out.resampled
    # fr_deepseq_resolve keeps its five arguments and Mandelbrot's rules for p
    walk = (C.c_char * 64)()
    pm = fr.FractalState(max_iterations=64).to_params(fr.FractalType.Mandelbrot, fr.Precision.F64, False)
    ps = fr.FractalState(max_iterations=64).to_params(fr.FractalType.BurningShip, fr.Precision.F64, False)
    d = K.fr_deep_sequence_desc(b"-2", b"0", b"1e-310", b"2.5e-311", 5, 0, 1, 0)
    assert L.fr_deepseq_resolve(C.byref(pm), C.byref(d), 64, 48, walk) == 0
    assert L.fr_deepseq_resolve(C.byref(ps), C.byref(d), 64, 48, walk) == K.FR_ERR_UNSUPPORTED
