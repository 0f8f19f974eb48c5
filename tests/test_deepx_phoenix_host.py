"""Deep Phoenix views below 1e-290 (fr_render_deepx_phoenix): the parts that need no GPU -- the header macro, the symbols and
their ctypes mirror, the validator's answers one by one, the extended reference orbit against Python integers and against the
fp64 and Mandelbrot orbits, and the two-mode restatement of the kernel's step against the direct fixed-point iteration on every
pixel of the four new views."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import deep_phoenix_ref as D
import deep_ref as R
import deepx_phoenix_ref as PX
import deepx_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = PX.GOLDEN_SIZE


def _view(fr, cx="-0.5", cy="0", zoom="1e-400", frac_bits=0, reserved=0):
    enc = lambda s: s.encode() if isinstance(s, str) else s
    return fr._capi.fr_deepx_view(enc(cx), enc(cy), enc(zoom), frac_bits, reserved)


def _orbit(fr, v, F=0):
    return fr.deepx_phoenix_reference_orbit(fr.DeepView(v["cx"], v["cy"], F, zoom=v["zoom"]), v["max_iter"],
                                            fr.PhoenixParams(phoenix_p=v["p"], phoenix_r=v["r"]))


def _same_orbit(got, want):
    return (got[0].shape == want[0].shape and np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64))
            and np.array_equal(got[1], want[1]))


# ---- ABI -----------------------------------------------------------------------------------------------------------
def test_header_macro_symbols_and_mirror(fr, tmp_path):
    names = ("fr_deepx_phoenix_validate", "fr_deepx_phoenix_reference_orbit", "fr_render_deepx_phoenix",
             "fr_render_deepx_phoenix_async")
    for n in names:
        assert n in fr._capi.SIGNATURES, n
        assert getattr(fr.lib(), n) is not None
    assert callable(fr.Renderer.render_deepx_phoenix) and callable(fr.deepx_phoenix_reference_orbit)
    assert "deepx_phoenix_reference_orbit" in fr.__all__
    with open(os.path.join(ROOT, "include", "fractalrenderer_amd.h")) as f:
        header = f.read()
    for n in names:
        assert header.count(n + "(") == 1, n
    gcc = shutil.which("gcc")
    if gcc:                                   # the macro, and the prototypes as a C compiler reads them
        src = tmp_path / "phoenixx.c"
        src.write_text('#include "fractalrenderer_amd.h"\n'
                       "#if !defined(FR_HAS_DEEPX_PHOENIX) || FR_HAS_DEEPX_PHOENIX != 1\n#error FR_HAS_DEEPX_PHOENIX\n#endif\n"
                       "int (*v)(const fr_params*, const fr_phoenix_params*, const fr_deepx_view*, uint32_t, uint32_t)\n"
                       "    = fr_deepx_phoenix_validate;\n"
                       "int (*a)(const fr_deepx_view*, const fr_phoenix_params*, int32_t, double*, int32_t*, int32_t*)\n"
                       "    = fr_deepx_phoenix_reference_orbit;\n"
                       "int (*b)(fr_ctx*, const fr_params*, const fr_phoenix_params*, const fr_deepx_view*, uint32_t, uint32_t,\n"
                       "         const fr_shard*, const fr_output*) = fr_render_deepx_phoenix;\n"
                       "int (*c)(fr_ctx*, const fr_params*, const fr_phoenix_params*, const fr_deepx_view*, uint32_t, uint32_t,\n"
                       "         const fr_shard*, const fr_output*, void*) = fr_render_deepx_phoenix_async;\n")
        subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "phoenixx.o")], check=True)
    else:
        assert "#define FR_HAS_DEEPX_PHOENIX 1" in header


# ---- the validator, one answer at a time, in fr_deep_phoenix_validate's order ------------------------------------------------
def _validator(fr):
    F = fr._capi
    L = fr.lib()
    good = _view(fr, PX.PX400A["cx"], PX.PX400A["cy"])

    def check(W=64, H=48, view=good, ph=(0.0, -0.5, 0, 0), **kw):
        p = fr.FractalState(zoom=1e-30).to_params(fr.FractalType.Phoenix, fr.Precision.F64)
        for k, val in kw.items():
            setattr(p, k, val)
        php = F.fr_phoenix_params(*ph)
        return L.fr_deepx_phoenix_validate(C.byref(p), C.byref(php), C.byref(view), W, H)

    return check


def test_validator_accepts_and_ignores_what_it_does_not_read(fr):
    F = fr._capi
    check = _validator(fr)
    assert check() == F.FR_OK
    assert check(flags=1) == F.FR_OK                     # FR_FLAG_POST_CHAIN
    assert check(bailout=float("nan")) == F.FR_OK and check(color_offset=float("nan")) == F.FR_OK
    assert check(interior_style=3) == F.FR_OK and check(orbit_trap_enabled=1) == F.FR_OK and check(use_perturbation=1) == F.FR_OK
    assert check(center_x=float("nan"), center_y=float("inf")) == F.FR_OK       # the double centre is not read
    for z in (1e-300, 0.0, float("nan"), -1.0, 1e9):                            # nor is p->zoom: the view's string is the zoom
        assert check(zoom=z) == F.FR_OK, z
    assert check(max_iterations=1 << 24, antialiasing_samples=16) == F.FR_OK
    assert check(ph=(0.25, -0.375, 0, 0)) == F.FR_OK and check(ph=(-(2.0 ** 31), 2.0 ** 31, 0, 0)) == F.FR_OK


def test_validator_null_arguments(fr):
    F = fr._capi
    L = fr.lib()
    good = _view(fr, "0", "0")
    p = fr.FractalState().to_params(fr.FractalType.Phoenix, fr.Precision.F64)
    ph = F.fr_phoenix_params(0.0, -0.5, 0, 0)
    assert L.fr_deepx_phoenix_validate(None, C.byref(ph), C.byref(good), 64, 48) == F.FR_ERR_INVALID_ARG
    assert L.fr_deepx_phoenix_validate(C.byref(p), None, C.byref(good), 64, 48) == F.FR_ERR_INVALID_ARG
    assert L.fr_deepx_phoenix_validate(C.byref(p), C.byref(ph), None, 64, 48) == F.FR_ERR_INVALID_ARG
    # the render entry points: a NULL context, params, phoenix params, view or output
    o = F.fr_output(None, None, None, F.FR_MEM_HOST, 0)
    assert L.fr_render_deepx_phoenix(None, C.byref(p), C.byref(ph), C.byref(good), 64, 48, None, C.byref(o)) == F.FR_ERR_INVALID_ARG
    assert L.fr_render_deepx_phoenix_async(None, C.byref(p), C.byref(ph), C.byref(good), 64, 48, None, C.byref(o),
                                           None) == F.FR_ERR_INVALID_ARG


def test_validator_fractal_type_and_precision_come_first(fr):
    F = fr._capi
    check = _validator(fr)
    for t in (0, 1, 2, 3, 5, 99):
        assert check(fractal_type=t) == F.FR_ERR_UNSUPPORTED, t
    assert check(precision=0) == F.FR_ERR_UNSUPPORTED and check(precision=7) == F.FR_ERR_UNSUPPORTED
    assert check(fractal_type=0, W=0) == F.FR_ERR_UNSUPPORTED
    assert check(precision=0, max_iterations=0) == F.FR_ERR_UNSUPPORTED


def test_validator_fields_phoenix_reads_then_p_and_r(fr):
    F = fr._capi
    L = fr.lib()
    check = _validator(fr)
    for kw in (dict(W=0), dict(H=0), dict(W=65536, H=32768), dict(max_iterations=0), dict(max_iterations=(1 << 24) + 1),
               dict(antialiasing_samples=17), dict(antialiasing_samples=-1), dict(julia_c_real=float("inf")),
               dict(julia_c_imag=float("nan"))):
        assert check(**kw) == F.FR_ERR_INVALID_ARG, kw
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert check(ph=(bad, -0.5, 0, 0)) == F.FR_ERR_INVALID_ARG, bad
        assert check(ph=(0.0, bad, 0, 0)) == F.FR_ERR_INVALID_ARG, bad
    assert check(ph=(0.0, -0.5, 0, 1)) == F.FR_ERR_INVALID_ARG                  # reserved
    assert check(ph=(0.0, -0.5, 2, 0)) == F.FR_ERR_INVALID_ARG                  # use_julia_set is a bool
    assert check(ph=(2.0 ** 32, -0.5, 0, 0)) == F.FR_ERR_INVALID_ARG            # the fixed point's range
    assert check(ph=(0.0, -(2.0 ** 32), 0, 0)) == F.FR_ERR_INVALID_ARG
    assert "2^32" in L.fr_last_error().decode()
    # a field rule comes before the rules behind it: Julia mode, a BLA flag, a bad view
    assert check(max_iterations=0, ph=(0.0, -0.5, 1, 0)) == F.FR_ERR_INVALID_ARG
    assert check(ph=(2.0 ** 32, -0.5, 1, 0), flags=F.FR_FLAG_DEEPX_BLA) == F.FR_ERR_INVALID_ARG


def test_validator_julia_mode_is_unsupported_and_says_why(fr):
    F = fr._capi
    L = fr.lib()
    check = _validator(fr)
    assert check(ph=(0.0, -0.5, 1, 0)) == F.FR_ERR_UNSUPPORTED
    msg = L.fr_last_error().decode()
    assert "use_julia_set" in msg and "one colour" in msg and "fr_render_deepx_phoenix" in msg
    assert check(ph=(0.0, -0.5, 1, 0), view=_view(fr, "x", "0")) == F.FR_ERR_UNSUPPORTED     # ... before the view


def test_validator_every_bla_flag_is_unsupported_before_the_view_strings(fr):
    F = fr._capi
    L = fr.lib()
    check = _validator(fr)
    for flag in (F.FR_FLAG_DEEP_BLA, F.FR_FLAG_DEEPX_BLA, F.FR_FLAG_DEEP_SHIP_BLA, F.FR_FLAG_DEEPX_SHIP_BLA,
                 F.FR_FLAG_DEEP_JULIA_BLA, F.FR_FLAG_DEEPX_JULIA_BLA):
        assert check(flags=flag) == F.FR_ERR_UNSUPPORTED, flag
        msg = L.fr_last_error().decode()
        assert "BLA" in msg and "fr_render_deepx_phoenix" in msg
        assert check(flags=flag | 1) == F.FR_ERR_UNSUPPORTED, flag
        assert check(flags=flag, view=_view(fr, "1e", "0")) == F.FR_ERR_UNSUPPORTED, flag
        assert check(flags=flag, view=_view(fr, "0", "0", "1e-2000")) == F.FR_ERR_UNSUPPORTED, flag


def test_validator_view_as_fr_deepx_validate_checks_it(fr):
    F = fr._capi
    L = fr.lib()
    check = _validator(fr)
    bad_views = [_view(fr, "1e", "0"), _view(fr, "0", "x"), _view(fr, "0", "0", "1e-400", 0, 3), _view(fr, "0", "0", "1e-400", 100),
                 _view(fr, "0", "0", "1e-400", 4097), _view(fr, "1" * 4097, "0"), _view(fr, "4294967296", "0"), _view(fr, None, "0"),
                 _view(fr, "0", "0", None), _view(fr, "0", "0", ""), _view(fr, "0", "0", "-1e-30"), _view(fr, "0", "0", "0"),
                 _view(fr, "0", "0", "abc")]
    mandel = fr.FractalState().to_params(fr.FractalType.Mandelbrot, fr.Precision.F64)
    for v in bad_views:
        assert check(view=v) == F.FR_ERR_INVALID_ARG
        assert L.fr_deepx_validate(C.byref(mandel), C.byref(v), 64, 48) == F.FR_ERR_INVALID_ARG      # the same answer
    assert check(view=_view(fr, "0", "0", "1e-400", 128)) == F.FR_OK and check(view=_view(fr, "0", "0", "1e-400", 4096)) == F.FR_OK
    # the zoom range, compared on the rounded pair: its edges
    for z in ("1e-1000", "1e3", "1000", "3", "1e-290", "1e-291"):
        assert check(view=_view(fr, "0", "0", z)) == F.FR_OK, z
    for z in ("9.999999999e-1001", "1000.0000001", "1e-1001", "1e4"):
        assert check(view=_view(fr, "0", "0", z)) == F.FR_ERR_INVALID_ARG, z


def test_the_other_entry_points_are_as_they_were(fr):
    """fr_deep_phoenix_validate still refuses a zoom below 1e-290, and the extended validators still refuse Phoenix"""
    F = fr._capi
    L = fr.lib()
    p = fr.FractalState(zoom=1e-291).to_params(fr.FractalType.Phoenix, fr.Precision.F64)
    ph = F.fr_phoenix_params(0.0, -0.5, 0, 0)
    v = F.fr_deep_view(b"0", b"0", 0, 0)
    assert L.fr_deep_phoenix_validate(C.byref(p), C.byref(ph), C.byref(v), 64, 48) == F.FR_ERR_INVALID_ARG
    vx = _view(fr, "0", "0", "1e-400")
    for fn in (L.fr_deepx_validate, L.fr_deepx_ship_validate):
        assert fn(C.byref(p), C.byref(vx), 64, 48) == F.FR_ERR_UNSUPPORTED


def test_python_method_needs_a_zoom_string(fr):
    with pytest.raises(ValueError, match="zoom string"):
        fr.Renderer.render_deepx_phoenix(None, fr.FractalState(), 8, 8, fr.DeepView("0", "0"))
    with pytest.raises(ValueError, match="zoom string"):
        fr.Renderer.render_deepx_phoenix(None, fr.FractalState(), 8, 8, None)


# ---- the reference orbit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PX.NEW_VIEWS))
def test_reference_orbit_is_bitwise_the_python_int_orbit(fr, name):
    v = PX.NEW_VIEWS[name]
    got, want = _orbit(fr, v), PX.orbit_of(v)
    assert _same_orbit(got, want)
    assert got[1][0] == X.X_ZERO and len(got[1]) - 1 <= v["max_iter"]
    print(name, "N", len(got[1]) - 1, "F", PX.frac_bits_of(v))


@pytest.mark.parametrize("name", ["PA", "PB30"])
def test_reference_orbit_equals_the_fp64_entry_points(fr, name):
    v = D.VIEWS[name]
    mant, exp2 = _orbit(fr, PX.OLD_VIEWS[name])
    want = fr.deep_phoenix_reference_orbit(fr.DeepView(v["cx"], v["cy"]), v["zoom"], v["max_iter"],
                                           fr.PhoenixParams(phoenix_p=v["p"], phoenix_r=v["r"]))
    assert len(want) - 1 == D.ORBIT_N[name]
    assert np.all(exp2[1:] == 0) and exp2[0] == X.X_ZERO             # every point but Z_0 is a normal double
    assert mant.shape == want.shape and np.array_equal(mant.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("name", ["A", "B"])
def test_reference_orbit_at_p_r_zero_is_fr_deepx_reference_orbit_at_bailout_2(fr, name):
    v = R.VIEWS[name]
    view = fr.DeepView(v["cx"], v["cy"], zoom=repr(float(v["zoom"])))
    got = fr.deepx_phoenix_reference_orbit(view, v["max_iter"], fr.PhoenixParams(phoenix_p=0.0, phoenix_r=0.0))
    want = fr.deepx_reference_orbit(view, v["max_iter"], 2.0)
    assert len(got[1]) > 100 and _same_orbit(got, want)


def test_orbit_entry_validation_and_null_arguments(fr):
    F = fr._capi
    L = fr.lib()
    good = _view(fr, "-0.5", "0", "1e-400")
    mant = np.empty((101, 2), np.float64)
    exp2 = np.empty(101, np.int32)
    n = C.c_int32()

    def orbit(v, it=100, p=0.0, r=-0.5):
        ph = F.fr_phoenix_params(p, r, 0, 0)
        return L.fr_deepx_phoenix_reference_orbit(C.byref(v), C.byref(ph), it, mant.ctypes.data, exp2.ctypes.data, C.byref(n))

    assert orbit(good) == F.FR_OK and n.value == 101
    for v in (_view(fr, "1e", "0"), _view(fr, "0", "0", "1e-1001"), _view(fr, "0", "0", "1e-400", 0, 1), _view(fr, "0", "0", None)):
        assert orbit(v) == F.FR_ERR_INVALID_ARG
    for it in (0, -1, (1 << 24) + 1):
        assert orbit(good, it=it) == F.FR_ERR_INVALID_ARG, it
    for bad in (float("inf"), float("nan"), 2.0 ** 32):
        assert orbit(good, p=bad) == F.FR_ERR_INVALID_ARG and orbit(good, r=bad) == F.FR_ERR_INVALID_ARG, bad
    ph = F.fr_phoenix_params(0.0, -0.5, 0, 0)
    args = [C.byref(good), C.byref(ph), 100, mant.ctypes.data, exp2.ctypes.data, C.byref(n)]
    for k in (0, 1, 3, 4, 5):
        a = list(args)
        a[k] = None
        assert L.fr_deepx_phoenix_reference_orbit(*a) == F.FR_ERR_INVALID_ARG, k


# ---- the restatement against the direct fixed-point iteration -------------------------------------------------------
@pytest.fixture(scope="module")
def restated(fr):
    """every new view at 24x18, aa 1, on the library's orbit: name -> (iter, stats), computed once"""
    out = {}
    for name, v in PX.NEW_VIEWS.items():
        st = {}
        it = PX.restate_x(v, W, H, orbit=_orbit(fr, v), stats=st)[0]
        out[name] = (it, st)
    return out


@pytest.fixture(scope="module")
def exact():
    return PX.exact_golden()


@pytest.mark.parametrize("name", list(PX.NEW_VIEWS))
def test_recorded_exact_frames_are_the_exact_iteration(exact, name):
    """tests/golden/deepx_phoenix_exact.npz against exact_iter_x on a sample of its pixels (the whole frame takes 10 to 40 s:
    tests/golden/make_deepx_phoenix_golden.py): the corners, the centre, and one pixel per escape index that occurs"""
    v = PX.NEW_VIEWS[name]
    ex = exact[name]
    assert ex.shape == (H, W) and ex.dtype == np.int32
    pixels = {(0, 0), (H - 1, W - 1), (0, W - 1), (H // 2, W // 2)}
    for val in np.unique(ex)[::3]:
        y, x = np.argwhere(ex == val)[0]
        pixels.add((int(y), int(x)))
    for y, x in sorted(pixels):
        assert PX.exact_iter_x(v, x, y, W, H) == ex[y, x], (name, x, y)


@pytest.mark.parametrize("name", list(PX.NEW_VIEWS))
def test_restatement_iter_is_the_exact_iteration_on_every_pixel(restated, exact, name):
    v = PX.NEW_VIEWS[name]
    it, _ = restated[name]
    ex = exact[name]
    distinct = len(np.unique(ex[ex < v["max_iter"]]))
    interior = float((ex == v["max_iter"]).mean())
    print(name, "mismatches", int((it != ex).sum()), "distinct escape indices", distinct, "interior share", interior)
    # conditions on the exact iteration alone: the frame is a real one
    assert distinct >= 8
    if name == "TIP1000":
        assert (ex == v["max_iter"]).sum() >= 1
    else:
        assert 0.1 <= interior <= 0.9
    assert np.array_equal(it, ex), f"{int((it != ex).sum())} of {it.size} pixels differ"


@pytest.mark.parametrize("name", list(PX.NEW_VIEWS))
def test_restatement_lanes_change_mode_and_rebase(restated, name):
    st = restated[name][1]
    print(name, st)
    assert st["ext_steps"] > 0 and st["plain_steps"] > 0 and st["to_plain"] > 0
    assert st["rebases"] > 0


def test_tip1000_pins_the_exponent_range(fr):
    """the deltas start at 2^-3322 and stay extended for more than a thousand updates"""
    v = PX.TIP1000
    zm, ze = X.zoom_pair(v["zoom"])
    assert ze == -3322
    st = {}
    PX.restate_x(v, 8, 6, orbit=_orbit(fr, v), stats=st)
    assert st["ext_steps"] >= 1000 * 40                          # most of the 48 samples, > 1000 updates each


@pytest.mark.parametrize("name", ["PA30", "PB30", "PA", "PB", "shallowA", "miniR"])
def test_restatement_on_fp64_views_is_the_fp64_restatement_bit_for_bit(fr, name):
    """an extended view whose zoom string names a double: iter, nu and rgb of deep_phoenix_ref.restate"""
    v = D.VIEWS[name]
    st = {}
    it, nu, rgb = PX.restate_x(PX.OLD_VIEWS[name], W, H, aa=2, density=10.0, post=True, orbit=_orbit(fr, PX.OLD_VIEWS[name]), stats=st)
    it0, nu0, rgb0, _, _ = D.restate(v, W, H, aa=2, density=10.0, post=True)
    assert np.array_equal(it, it0)
    assert np.array_equal(nu.view(np.uint64), nu0.view(np.uint64))
    assert np.array_equal(rgb.view(np.uint32), rgb0.view(np.uint32))
    assert st["to_ext"] == 0 and st["plain_steps"] > st["ext_steps"] > 0      # extended for the first update(s) only
