"""Deep Phoenix views (fr_render_deep_phoenix): the parts that need no GPU -- the header macro, the symbols and their ctypes
mirror, the fixed-point reference orbit against Python integers, the validator's answers one by one, and the fp64 restatement of
the kernel's step against the direct fixed-point iteration on every pixel of every view of deep_phoenix_ref."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import deep_phoenix_ref as D
import deep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 24, 18


def _view(fr, cx="-0.5", cy="0", frac_bits=0, reserved=0):
    return fr._capi.fr_deep_view(cx.encode() if isinstance(cx, str) else cx, cy.encode() if isinstance(cy, str) else cy,
                                 frac_bits, reserved)


def _orbit(fr, v, F=0):
    return fr.deep_phoenix_reference_orbit(fr.DeepView(v["cx"], v["cy"], F), v["zoom"], v["max_iter"],
                                           fr.PhoenixParams(phoenix_p=v["p"], phoenix_r=v["r"]))


# ---- ABI -----------------------------------------------------------------------------------------------------------
def test_header_macro_symbols_and_mirror(fr, tmp_path):
    names = ("fr_deep_phoenix_validate", "fr_deep_phoenix_reference_orbit", "fr_render_deep_phoenix", "fr_render_deep_phoenix_async")
    for n in names:
        assert n in fr._capi.SIGNATURES, n
        assert getattr(fr.lib(), n) is not None
    assert callable(fr.Renderer.render_deep_phoenix) and callable(fr.deep_phoenix_reference_orbit)
    with open(os.path.join(ROOT, "include", "fractalrenderer_amd.h")) as f:
        header = f.read()
    for n in names:
        assert header.count(n + "(") == 1, n
    gcc = shutil.which("gcc")
    if gcc:                                   # the macro, and the prototypes as a C compiler reads them
        src = tmp_path / "phoenix.c"
        src.write_text('#include "fractalrenderer_amd.h"\n'
                       "#if !defined(FR_HAS_DEEP_PHOENIX) || FR_HAS_DEEP_PHOENIX != 1\n#error FR_HAS_DEEP_PHOENIX\n#endif\n"
                       "int (*v)(const fr_params*, const fr_phoenix_params*, const fr_deep_view*, uint32_t, uint32_t)\n"
                       "    = fr_deep_phoenix_validate;\n"
                       "int (*a)(const fr_deep_view*, const fr_phoenix_params*, double, int32_t, double*, int32_t*)\n"
                       "    = fr_deep_phoenix_reference_orbit;\n"
                       "int (*b)(fr_ctx*, const fr_params*, const fr_phoenix_params*, const fr_deep_view*, uint32_t, uint32_t,\n"
                       "         const fr_shard*, const fr_output*) = fr_render_deep_phoenix;\n"
                       "int (*c)(fr_ctx*, const fr_params*, const fr_phoenix_params*, const fr_deep_view*, uint32_t, uint32_t,\n"
                       "         const fr_shard*, const fr_output*, void*) = fr_render_deep_phoenix_async;\n")
        subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "phoenix.o")], check=True)
    else:
        assert "#define FR_HAS_DEEP_PHOENIX 1" in header


# ---- reference orbit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["PA30", "PB30", "PB"])
def test_reference_orbit_is_bitwise_the_python_int_orbit(fr, name):
    v = D.VIEWS[name]
    got = _orbit(fr, v)
    want = D.view_orbit(v)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert len(got) - 1 == D.ORBIT_N[name] < v["max_iter"]        # the reference escapes: rebases happen by m == N


def test_reference_orbit_other_parameters_and_explicit_bits(fr):
    """negative and positive p and r, p alone, values below 2^-F's reach of a float's last bit, explicit fraction bits"""
    for cx, cy, zoom, it, p, r, F in [("-0.5", "0.1", 1.0, 200, -0.1, -0.8, 0), ("0.2", "-0.3", 1e-5, 150, 0.2, -0.3, 130),
                                      ("-0.4", "0.2", 1e-20, 300, 0.56667, 0.25, 0), ("0.1", "0.1", 3.0, 100, 1e-42, -1e-40, 128),
                                      ("-1.0", "0.05", 1e-3, 250, -3.0e-39, 0.0, 128), ("3", "0", 3.0, 10, 0.0, -0.5, 0)]:
        v = dict(cx=cx, cy=cy, zoom=zoom, max_iter=it, p=p, r=r)
        got = _orbit(fr, v, F)
        want = D.reference_orbit(cx, cy, zoom, it, p, r, F)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (cx, cy, p, r, F)


@pytest.mark.parametrize("name", ["A", "B"])
def test_reference_orbit_at_p_r_zero_is_mandelbrots_at_bailout_2(fr, name):
    v = R.VIEWS[name]
    got = fr.deep_phoenix_reference_orbit(fr.DeepView(v["cx"], v["cy"]), v["zoom"], v["max_iter"],
                                          fr.PhoenixParams(phoenix_p=0.0, phoenix_r=0.0))
    want = fr.deep_reference_orbit(fr.DeepView(v["cx"], v["cy"]), v["zoom"], v["max_iter"], 2.0)
    assert got.shape == want.shape and len(got) > 100
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_orbit_entry_validation_and_null_arguments(fr):
    F = fr._capi
    L = fr.lib()
    good = _view(fr, D.PA30["cx"], D.PA30["cy"])
    buf = np.empty((1001, 2), np.float64)
    n = C.c_int32()

    def orbit(v, zoom=1e-30, it=1000, p=0.0, r=-0.5):
        ph = F.fr_phoenix_params(p, r, 0, 0)
        return L.fr_deep_phoenix_reference_orbit(C.byref(v), C.byref(ph), zoom, it, buf.ctypes.data, C.byref(n))

    assert orbit(good) == F.FR_OK
    for s in ("", "1e", "--1", "nan", "1" * 4097):
        assert orbit(_view(fr, s, "0")) == F.FR_ERR_INVALID_ARG, s
        assert orbit(_view(fr, "0", s)) == F.FR_ERR_INVALID_ARG, s
    assert orbit(_view(fr, None, "0")) == F.FR_ERR_INVALID_ARG
    assert orbit(_view(fr, "0", "0", 0, 1)) == F.FR_ERR_INVALID_ARG
    for bits in (1, 127, 4097, -128):
        assert orbit(_view(fr, "0", "0", bits)) == F.FR_ERR_INVALID_ARG, bits
    for z in (1e-291, 0.0, -1e-30, 1001.0, float("inf"), float("nan")):
        assert orbit(good, zoom=z) == F.FR_ERR_INVALID_ARG, z
    assert orbit(good, zoom=1e-290) == F.FR_OK and orbit(good, zoom=1e3) == F.FR_OK
    for it in (0, -1, (1 << 24) + 1):
        assert orbit(good, it=it) == F.FR_ERR_INVALID_ARG, it
    for bad in (float("inf"), float("nan"), 2.0 ** 32, -(2.0 ** 32)):
        assert orbit(good, p=bad) == F.FR_ERR_INVALID_ARG, bad
        assert orbit(good, r=bad) == F.FR_ERR_INVALID_ARG, bad
    assert orbit(good, it=4, p=2.0 ** 31, r=-(2.0 ** 31)) == F.FR_OK
    ph = F.fr_phoenix_params(0.0, -0.5, 0, 0)
    assert L.fr_deep_phoenix_reference_orbit(None, C.byref(ph), 1e-30, 100, buf.ctypes.data, C.byref(n)) == F.FR_ERR_INVALID_ARG
    assert L.fr_deep_phoenix_reference_orbit(C.byref(good), None, 1e-30, 100, buf.ctypes.data, C.byref(n)) == F.FR_ERR_INVALID_ARG
    assert L.fr_deep_phoenix_reference_orbit(C.byref(good), C.byref(ph), 1e-30, 100, None, C.byref(n)) == F.FR_ERR_INVALID_ARG
    assert L.fr_deep_phoenix_reference_orbit(C.byref(good), C.byref(ph), 1e-30, 100, buf.ctypes.data, None) == F.FR_ERR_INVALID_ARG

    # the render entry points: a NULL context, params, phoenix params, view or output is an invalid argument
    base = fr.FractalState(zoom=1e-30).to_params(fr.FractalType.Phoenix, fr.Precision.F64)
    o = F.fr_output(None, None, None, F.FR_MEM_HOST, 0)
    assert L.fr_render_deep_phoenix(None, C.byref(base), C.byref(ph), C.byref(good), 64, 48, None, C.byref(o)) == F.FR_ERR_INVALID_ARG
    assert L.fr_render_deep_phoenix_async(None, C.byref(base), C.byref(ph), C.byref(good), 64, 48, None, C.byref(o),
                                          None) == F.FR_ERR_INVALID_ARG


# ---- the validator, one answer at a time -----------------------------------------------------------------------------
def _validator(fr):
    F = fr._capi
    L = fr.lib()
    good = _view(fr, D.PA30["cx"], D.PA30["cy"])

    def check(W=64, H=48, view=good, ph=(0.0, -0.5, 0, 0), **kw):
        p = fr.FractalState(zoom=1e-30).to_params(fr.FractalType.Phoenix, fr.Precision.F64)
        for k, val in kw.items():
            setattr(p, k, val)
        php = F.fr_phoenix_params(*ph)
        return L.fr_deep_phoenix_validate(C.byref(p), C.byref(php), C.byref(view), W, H)

    return check


def test_validator_accepts_and_ignores_what_phoenix_ignores(fr):
    F = fr._capi
    check = _validator(fr)
    assert check() == F.FR_OK
    assert check(flags=1) == F.FR_OK                     # FR_FLAG_POST_CHAIN
    # not read by the Phoenix shader: no rule
    assert check(bailout=0.0) == F.FR_OK and check(bailout=float("nan")) == F.FR_OK and check(bailout=1e9) == F.FR_OK
    assert check(color_offset=float("nan")) == F.FR_OK
    assert check(interior_style=3) == F.FR_OK and check(orbit_trap_enabled=1) == F.FR_OK
    assert check(stripe_enabled=1, interior_style=2) == F.FR_OK
    assert check(use_perturbation=1) == F.FR_OK
    assert check(center_x=float("nan"), center_y=float("inf")) == F.FR_OK       # the double centre is not read
    assert check(max_iterations=1 << 24, antialiasing_samples=16, zoom=1e-290) == F.FR_OK
    assert check(zoom=1e3) == F.FR_OK
    assert check(ph=(0.25, -0.375, 0, 0)) == F.FR_OK and check(ph=(-(2.0 ** 31), 2.0 ** 31, 0, 0)) == F.FR_OK


def test_validator_fractal_type_and_precision_are_unsupported(fr):
    F = fr._capi
    check = _validator(fr)
    for t in (0, 1, 2, 3, 5, 99):
        assert check(fractal_type=t) == F.FR_ERR_UNSUPPORTED, t
    assert check(precision=0) == F.FR_ERR_UNSUPPORTED
    assert check(precision=7) == F.FR_ERR_UNSUPPORTED
    # ... and come first: a bad frame or field behind a foreign fractal type is still "unsupported"
    assert check(fractal_type=0, W=0) == F.FR_ERR_UNSUPPORTED
    assert check(precision=0, max_iterations=0) == F.FR_ERR_UNSUPPORTED


def test_validator_fields_phoenix_reads(fr):
    F = fr._capi
    check = _validator(fr)
    for kw in (dict(W=0), dict(H=0), dict(W=65536, H=32768), dict(max_iterations=0), dict(max_iterations=(1 << 24) + 1),
               dict(antialiasing_samples=17), dict(antialiasing_samples=-1), dict(julia_c_real=float("inf")),
               dict(julia_c_imag=float("nan")), dict(zoom=float("nan")), dict(zoom=0.0)):
        assert check(**kw) == F.FR_ERR_INVALID_ARG, kw


def test_validator_phoenix_params(fr):
    F = fr._capi
    L = fr.lib()
    check = _validator(fr)
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert check(ph=(bad, -0.5, 0, 0)) == F.FR_ERR_INVALID_ARG, bad
        assert check(ph=(0.0, bad, 0, 0)) == F.FR_ERR_INVALID_ARG, bad
    assert check(ph=(0.0, -0.5, 0, 1)) == F.FR_ERR_INVALID_ARG                  # reserved
    assert check(ph=(0.0, -0.5, 2, 0)) == F.FR_ERR_INVALID_ARG                  # use_julia_set is a bool
    assert check(ph=(2.0 ** 32, -0.5, 0, 0)) == F.FR_ERR_INVALID_ARG            # the fixed point's range
    assert check(ph=(0.0, -(2.0 ** 32), 0, 0)) == F.FR_ERR_INVALID_ARG
    assert "2^32" in L.fr_last_error().decode()


def test_validator_julia_mode_is_unsupported_and_says_why(fr):
    F = fr._capi
    L = fr.lib()
    check = _validator(fr)
    assert check(ph=(0.0, -0.5, 1, 0)) == F.FR_ERR_UNSUPPORTED
    msg = L.fr_last_error().decode()
    assert "use_julia_set" in msg and "one colour" in msg


def test_validator_zoom_range(fr):
    F = fr._capi
    check = _validator(fr)
    for z in (1e-291, 1001.0, -1e-30, float("inf")):
        assert check(zoom=z) == F.FR_ERR_INVALID_ARG, z
    assert check(zoom=1e-290) == F.FR_OK and check(zoom=1e3) == F.FR_OK


def test_validator_view(fr):
    F = fr._capi
    check = _validator(fr)
    assert check(view=_view(fr, "1e", "0")) == F.FR_ERR_INVALID_ARG
    assert check(view=_view(fr, "0", "x")) == F.FR_ERR_INVALID_ARG
    assert check(view=_view(fr, "0", "0", 0, 3)) == F.FR_ERR_INVALID_ARG        # reserved
    assert check(view=_view(fr, "0", "0", 100)) == F.FR_ERR_INVALID_ARG         # frac_bits
    assert check(view=_view(fr, "0", "0", 4097)) == F.FR_ERR_INVALID_ARG
    assert check(view=_view(fr, "0", "0", 128)) == F.FR_OK and check(view=_view(fr, "0", "0", 4096)) == F.FR_OK
    assert check(view=_view(fr, "1" * 4097, "0")) == F.FR_ERR_INVALID_ARG
    assert check(view=_view(fr, "4294967296", "0")) == F.FR_ERR_INVALID_ARG
    assert check(view=_view(fr, None, "0")) == F.FR_ERR_INVALID_ARG


def test_validator_every_bla_flag_is_unsupported_and_says_so(fr):
    F = fr._capi
    L = fr.lib()
    check = _validator(fr)
    for flag in (F.FR_FLAG_DEEP_BLA, F.FR_FLAG_DEEPX_BLA, F.FR_FLAG_DEEP_SHIP_BLA, F.FR_FLAG_DEEPX_SHIP_BLA,
                 F.FR_FLAG_DEEP_JULIA_BLA, F.FR_FLAG_DEEPX_JULIA_BLA):
        assert check(flags=flag) == F.FR_ERR_UNSUPPORTED, flag
        assert "BLA" in L.fr_last_error().decode()
        assert check(flags=flag | 1) == F.FR_ERR_UNSUPPORTED, flag


def test_validator_null_arguments(fr):
    F = fr._capi
    L = fr.lib()
    good = _view(fr, "0", "0")
    p = fr.FractalState(zoom=1e-30).to_params(fr.FractalType.Phoenix, fr.Precision.F64)
    ph = F.fr_phoenix_params(0.0, -0.5, 0, 0)
    assert L.fr_deep_phoenix_validate(None, C.byref(ph), C.byref(good), 64, 48) == F.FR_ERR_INVALID_ARG
    assert L.fr_deep_phoenix_validate(C.byref(p), None, C.byref(good), 64, 48) == F.FR_ERR_INVALID_ARG
    assert L.fr_deep_phoenix_validate(C.byref(p), C.byref(ph), None, 64, 48) == F.FR_ERR_INVALID_ARG


def test_existing_validators_still_refuse_phoenix(fr):
    """none of the other deep validators, nor fr_params_validate, has learnt about Phoenix"""
    F = fr._capi
    L = fr.lib()
    v = _view(fr, "0", "0")
    vx = F.fr_deepx_view(b"0", b"0", b"1e-30", 0, 0)
    p = fr.FractalState(zoom=1e-30).to_params(fr.FractalType.Phoenix, fr.Precision.F64)
    L.fr_deep_validate.restype = C.c_int
    L.fr_deep_validate.argtypes = [C.POINTER(F.fr_params), C.POINTER(F.fr_deep_view), C.c_uint32, C.c_uint32]
    L.fr_deep_julia_validate.restype = C.c_int
    L.fr_deep_julia_validate.argtypes = L.fr_deep_validate.argtypes
    for fn in (L.fr_deep_validate, L.fr_deep_ship_validate, L.fr_deep_julia_validate):
        assert fn(C.byref(p), C.byref(v), 64, 48) == F.FR_ERR_UNSUPPORTED
    for fn in (L.fr_deepx_validate, L.fr_deepx_ship_validate):
        assert fn(C.byref(p), C.byref(vx), 64, 48) == F.FR_ERR_UNSUPPORTED
    e = F.fr_deep_de(None, None, 0, 1.8)
    assert L.fr_deep_ship_de_validate(C.byref(p), C.byref(v), C.byref(e), 64, 48) == F.FR_ERR_UNSUPPORTED
    assert L.fr_params_validate(C.byref(p), 64, 48) == F.FR_ERR_UNSUPPORTED


def test_python_method_rejects_a_zoom_string(fr):
    with pytest.raises(ValueError, match="zoom"):
        fr.Renderer.render_deep_phoenix(None, fr.FractalState(), 8, 8, fr.DeepView("0", "0", zoom="1e-400"))


# ---- the restatement against the direct fixed-point iteration -------------------------------------------------------
@pytest.fixture(scope="module")
def restated(fr):
    """every view at 24x18, aa 1, on the library's orbit: name -> (iter, rebases), computed once"""
    out = {}
    for name, v in D.VIEWS.items():
        it, _, _, _, rebases = D.restate(v, W, H, orbit=_orbit(fr, v))
        out[name] = (it, rebases)
    return out


@pytest.mark.parametrize("name", list(D.VIEWS))
def test_restatement_iter_is_the_exact_iteration_on_every_pixel(restated, name):
    v = D.VIEWS[name]
    it, _ = restated[name]
    ex = D.exact_frame(v, W, H)
    assert np.array_equal(it, ex), f"{int((it != ex).sum())} of {it.size} pixels differ"
    # the frame is a real one: interior pixels next to many escape bands
    assert (ex == v["max_iter"]).sum() >= 40 and len(np.unique(ex)) >= 17


@pytest.mark.parametrize("name", list(D.DEEP_VIEWS))
def test_restatement_rebases_on_the_deep_views(restated, name):
    assert restated[name][1] > 0
    assert restated[name][1] >= 1000            # 1.2 k (PB) to 25 k (PA30) per frame


def test_rule_at_r_zero_is_mandelbrots(fr):
    """at p = r = 0 the step, the rebase rule and so every (iter, r2) are deep_ref.perturb's, bit for bit"""
    import deep_ship_ref as S
    v = D.MINI_0
    orbit = _orbit(fr, v)
    dcx, dcy = S.sample_dc(W, H, v["zoom"], 1, 0)
    it, r2, _, _, rebases = D.perturb(orbit, dcx, dcy, v["max_iter"], 0.0, 0.0)
    it_m, r2_m, rebases_m = R.perturb(orbit, dcx, dcy, v["max_iter"], 2.0)
    assert np.array_equal(it, it_m) and np.array_equal(r2.view(np.uint64), r2_m.view(np.uint64)) and rebases == rebases_m


def test_restated_colour_against_itself_leaves_nothing_out():
    """the rgba check of the GPU test (1e-4 on all but _few's share) holds with no exception at all when the restatement meets
    itself: the tolerance leaves room for the device's transcendentals only"""
    v = D.PA30
    a = D.restate(v, W, H, aa=2, density=10.0, post=True)[2]
    b = D.restate(v, W, H, aa=2, density=10.0, post=True)[2]
    assert np.array_equal(a, b)
