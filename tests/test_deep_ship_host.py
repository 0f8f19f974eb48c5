"""Deep Burning Ship views (fr_render_deep_ship): the parts that need no GPU -- the header macro, the symbols and their
ctypes mirror, the fixed-point reference orbit against Python integers, validation, NULL arguments, and the fp64
restatement of the kernel's step against the direct fixed-point iteration."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import deep_ship_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _view(fr, cx="-0.5", cy="0", frac_bits=0, reserved=0):
    return fr._capi.fr_deep_view(cx.encode() if isinstance(cx, str) else cx, cy.encode() if isinstance(cy, str) else cy,
                                 frac_bits, reserved)


# ---- ABI -----------------------------------------------------------------------------------------------------------
def test_header_macro_symbols_and_mirror(fr, tmp_path):
    names = ("fr_deep_ship_reference_orbit", "fr_render_deep_ship", "fr_render_deep_ship_async")
    for n in names:
        assert n in fr._capi.SIGNATURES, n
        assert getattr(fr.lib(), n) is not None
    assert "fr_deep_ship_validate" in fr._capi.INTERNAL_SIGNATURES
    assert fr._capi.SIGNATURES["fr_render_deep_ship"] == fr._capi.SIGNATURES["fr_render_deep"]
    assert fr._capi.SIGNATURES["fr_render_deep_ship_async"] == fr._capi.SIGNATURES["fr_render_deep_async"]
    assert fr._capi.SIGNATURES["fr_deep_ship_reference_orbit"] == fr._capi.SIGNATURES["fr_deep_reference_orbit"]
    assert callable(fr.Renderer.render_deep_ship) and callable(fr.deep_ship_reference_orbit)
    with open(os.path.join(ROOT, "include", "fractalrenderer_amd.h")) as f:
        header = f.read()
    for n in names:
        assert header.count(n + "(") == 1, n
    gcc = shutil.which("gcc")
    if gcc:                                   # the macro, and the prototypes as a C compiler reads them
        src = tmp_path / "ship.c"
        src.write_text('#include "fractalrenderer_amd.h"\n'
                       "#if !defined(FR_HAS_DEEP_SHIP) || FR_HAS_DEEP_SHIP != 1\n#error FR_HAS_DEEP_SHIP\n#endif\n"
                       "int (*a)(const fr_deep_view*, double, int32_t, float, double*, int32_t*) = fr_deep_ship_reference_orbit;\n"
                       "int (*b)(fr_ctx*, const fr_params*, const fr_deep_view*, uint32_t, uint32_t, const fr_shard*,\n"
                       "         const fr_output*) = fr_render_deep_ship;\n"
                       "int (*c)(fr_ctx*, const fr_params*, const fr_deep_view*, uint32_t, uint32_t, const fr_shard*,\n"
                       "         const fr_output*, void*) = fr_render_deep_ship_async;\n")
        subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "ship.o")], check=True)
    else:
        assert "#define FR_HAS_DEEP_SHIP 1" in header


# ---- reference orbit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shallow", "needle", "A", "B"])
def test_reference_orbit_is_bitwise_the_python_int_orbit(fr, name):
    v = S.VIEWS[name]
    got = fr.deep_ship_reference_orbit(fr.DeepView(v["cx"], v["cy"]), v["zoom"], v["max_iter"])
    want = S.reference_orbit(v["cx"], v["cy"], v["zoom"], v["max_iter"])
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    if name == "A":
        assert len(got) - 1 == 197                    # this reference escapes: the m == N rebase is exercised early
    if name == "B":
        assert len(got) - 1 == v["max_iter"] == 590   # this one ends by m == N
    if name != "shallow":                             # (at -0.5 - 0.5i no product is ever negative)
        mand = fr.deep_reference_orbit(fr.DeepView(v["cx"], v["cy"]), v["zoom"], v["max_iter"])
        assert mand.shape != got.shape or not np.array_equal(mand, got)      # not Mandelbrot's orbit


def test_reference_orbit_explicit_bits_and_bailout(fr):
    for cx, cy, zoom, it, bail, F in [("-1.75", "-0.03", 1e-5, 300, 2.0, 130), ("0.3", "-0.5", 1.0, 50, 100.0, 256),
                                      ("-1.7869205526611640", "-0.0116847206583667", 1e-20, 500, 4.0, 0),
                                      ("-0.5", "-0.5", 1e-3, 200, 0.5, 128), (S.SHIP_A["cx"], S.SHIP_A["cy"], 1e-30, 200, 4.0, 320)]:
        got = fr.deep_ship_reference_orbit(fr.DeepView(cx, cy, F), zoom, it, bail)
        want = S.reference_orbit(cx, cy, zoom, it, bail, F)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (cx, cy, F)


# ---- validation ------------------------------------------------------------------------------------------------------
def test_orbit_entry_validation_and_null_arguments(fr):
    F = fr._capi
    L = fr.lib()
    good = _view(fr, S.SHIP_A["cx"], S.SHIP_A["cy"])
    buf = np.empty((1001, 2), np.float64)
    n = C.c_int32()

    def orbit(v, zoom=1e-30, it=1000, bail=4.0):
        return L.fr_deep_ship_reference_orbit(C.byref(v), zoom, it, bail, buf.ctypes.data, C.byref(n))

    assert orbit(good) == F.FR_OK
    for s in ("", "1e", "--1", "nan", "0x1p3", "1" * 4097):
        assert orbit(_view(fr, s, "0")) == F.FR_ERR_INVALID_ARG, s
        assert orbit(_view(fr, "0", s)) == F.FR_ERR_INVALID_ARG, s
    assert orbit(_view(fr, None, "0")) == F.FR_ERR_INVALID_ARG
    assert orbit(_view(fr, "0", "0", 0, 1)) == F.FR_ERR_INVALID_ARG
    for bits in (1, 64, 127, 4097, -128):
        assert orbit(_view(fr, "0", "0", bits)) == F.FR_ERR_INVALID_ARG, bits
    for z in (1e-291, 0.0, -1e-30, 1001.0, float("inf"), float("nan")):
        assert orbit(good, zoom=z) == F.FR_ERR_INVALID_ARG, z
    assert orbit(good, zoom=1e-290) == F.FR_OK and orbit(good, zoom=1e3) == F.FR_OK
    for it in (0, -1, (1 << 24) + 1):
        assert orbit(good, it=it) == F.FR_ERR_INVALID_ARG, it
    for b in (0.0, -1.0, 65537.0, float("inf"), float("nan")):
        assert orbit(good, bail=b) == F.FR_ERR_INVALID_ARG, b
    assert orbit(good, bail=65536.0) == F.FR_OK
    assert L.fr_deep_ship_reference_orbit(None, 1e-30, 100, 4.0, buf.ctypes.data, C.byref(n)) == F.FR_ERR_INVALID_ARG
    assert L.fr_deep_ship_reference_orbit(C.byref(good), 1e-30, 100, 4.0, None, C.byref(n)) == F.FR_ERR_INVALID_ARG
    assert L.fr_deep_ship_reference_orbit(C.byref(good), 1e-30, 100, 4.0, buf.ctypes.data, None) == F.FR_ERR_INVALID_ARG

    # the render entry points: a NULL context, params, view or output is an invalid argument
    base = fr.FractalState(zoom=1e-30).to_params(fr.FractalType.BurningShip, fr.Precision.F64)
    o = F.fr_output(None, None, None, F.FR_MEM_HOST, 0)
    assert L.fr_render_deep_ship(None, C.byref(base), C.byref(good), 64, 48, None, C.byref(o)) == F.FR_ERR_INVALID_ARG
    assert L.fr_render_deep_ship_async(None, C.byref(base), C.byref(good), 64, 48, None, C.byref(o), None) == F.FR_ERR_INVALID_ARG
    assert L.fr_deep_ship_validate(None, C.byref(good), 64, 48) == F.FR_ERR_INVALID_ARG
    assert L.fr_deep_ship_validate(C.byref(base), None, 64, 48) == F.FR_ERR_INVALID_ARG


def test_validation_of_params(fr):
    """fr_deep_ship_validate's verdicts, through the internal entry the render entry points call after their NULL checks"""
    F = fr._capi
    L = fr.lib()
    L.fr_deep_validate.restype = C.c_int
    L.fr_deep_validate.argtypes = [C.POINTER(F.fr_params), C.POINTER(F.fr_deep_view), C.c_uint32, C.c_uint32]
    good = _view(fr, S.SHIP_A["cx"], S.SHIP_A["cy"])

    def check(W=64, H=48, view=good, fn=L.fr_deep_ship_validate, **kw):
        p = fr.FractalState(zoom=1e-30).to_params(fr.FractalType.BurningShip, fr.Precision.F64)
        for k, val in kw.items():
            setattr(p, k, val)
        return fn(C.byref(p), C.byref(view), W, H)

    assert check() == F.FR_OK
    # fractal and precision; fr_render_deep's validation keeps rejecting the ship
    for t in (0, 1, 3, 4, 5, 99):
        assert check(fractal_type=t) == F.FR_ERR_UNSUPPORTED, t
    assert check(precision=0) == F.FR_ERR_UNSUPPORTED
    assert check(fn=L.fr_deep_validate) == F.FR_ERR_UNSUPPORTED
    assert check(fn=L.fr_deep_validate, fractal_type=0) == F.FR_OK
    # where the ship needs its effects kernel
    assert check(orbit_trap_enabled=1) == F.FR_ERR_UNSUPPORTED
    assert check(stripe_enabled=1, interior_style=2) == F.FR_ERR_UNSUPPORTED
    assert check(interior_style=3) == F.FR_ERR_UNSUPPORTED
    assert check(stripe_enabled=1) == F.FR_OK
    assert check(stripe_enabled=1, interior_style=1) == F.FR_OK
    assert check(interior_style=1) == F.FR_OK and check(interior_style=2) == F.FR_OK
    # BLA
    assert check(flags=F.FR_FLAG_DEEP_BLA) == F.FR_ERR_UNSUPPORTED
    assert check(flags=F.FR_FLAG_DEEPX_BLA) == F.FR_ERR_UNSUPPORTED
    assert check(flags=1) == F.FR_OK                     # FR_FLAG_POST_CHAIN
    # fr_params_validate's rules; the double centre is not read
    assert check(center_x=float("nan"), center_y=float("inf")) == F.FR_OK
    for kw in (dict(W=0), dict(H=0), dict(W=65536, H=32768), dict(max_iterations=0), dict(max_iterations=(1 << 24) + 1),
               dict(antialiasing_samples=17), dict(antialiasing_samples=-1), dict(bailout=0.0), dict(bailout=float("nan")),
               dict(bailout=65537.0), dict(zoom=1e-291), dict(zoom=1001.0), dict(zoom=-1e-30), dict(zoom=0.0),
               dict(julia_c_real=float("inf"))):
        assert check(**kw) == F.FR_ERR_INVALID_ARG, kw
    assert check(max_iterations=1 << 24, antialiasing_samples=16, bailout=65536.0, zoom=1e-290) == F.FR_OK
    assert check(zoom=1e3) == F.FR_OK
    # the view
    assert check(view=_view(fr, "1e", "0")) == F.FR_ERR_INVALID_ARG
    assert check(view=_view(fr, "0", "0", 0, 3)) == F.FR_ERR_INVALID_ARG
    assert check(view=_view(fr, "0", "0", 100)) == F.FR_ERR_INVALID_ARG
    assert check(view=_view(fr, "1" * 4097, "0")) == F.FR_ERR_INVALID_ARG


def test_python_method_rejects_a_zoom_string(fr):
    with pytest.raises(ValueError):
        fr.Renderer.render_deep_ship(None, fr.FractalState(), 8, 8, fr.DeepView("0", "0", zoom="1e-400"))


# ---- the restatement against the direct fixed-point iteration -------------------------------------------------------
def test_fold_is_the_difference_of_magnitudes():
    rng = np.random.default_rng(7)
    X = np.concatenate([rng.standard_normal(4000), [0.0, 0.0, 1.0, -1.0, 1.0, -1.0]])
    a = np.concatenate([rng.standard_normal(4000) * 10.0 ** rng.integers(-30, 1, 4000), [0.5, -0.5, -1.0, 1.0, -3.0, 3.0]])
    got = S.fold(X, a)
    from fractions import Fraction
    for x, d, g in zip(X[::40].tolist() + X[-6:].tolist(), a[::40].tolist() + a[-6:].tolist(), got[::40].tolist() + got[-6:].tolist()):
        want = abs(Fraction(x) + Fraction(d)) - abs(Fraction(x))
        assert abs(Fraction(g) - want) <= abs(want) * Fraction(1, 1 << 52), (x, d)


@pytest.mark.parametrize("name", ["A", "B"])
def test_restatement_agrees_with_exact_iteration(fr, name):
    """the step as specified, on the library's orbit, at the 256 random pixels of the GPU test: agreement >= 0.99, no exact
    value covers 60 % of them, 20-95 % escape, and the samples rebase"""
    v = S.VIEWS[name]
    W, H = 256, 192
    rng = np.random.default_rng(99)
    ys, xs = rng.integers(0, H, 256), rng.integers(0, W, 256)
    orbit = fr.deep_ship_reference_orbit(fr.DeepView(v["cx"], v["cy"]), v["zoom"], v["max_iter"])
    dcx, dcy = S.sample_dc(W, H, v["zoom"], 1, 0)
    it, _, rebases, folded = S.perturb(orbit, dcx[ys, xs], dcy[ys, xs], v["max_iter"])
    ex = np.array([S.exact_iter(v["cx"], v["cy"], int(x), int(y), W, H, v["zoom"], v["max_iter"]) for x, y in zip(xs, ys)])
    assert np.unique(ex, return_counts=True)[1].max() <= 0.60 * len(ex)
    assert (ex == it).mean() >= 0.99
    assert 0.20 <= (it < v["max_iter"]).mean() <= 0.95
    assert rebases >= len(ex) and folded >= len(ex)
