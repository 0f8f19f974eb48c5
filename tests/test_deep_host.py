"""Deep Mandelbrot views (fr_render_deep): the parts that need no GPU -- ABI layout and defaults, the automatic fraction
bits, the decimal parser, the fixed-point reference orbit against Python integers, validation, and the fp64
restatement of the kernel against the direct fixed-point iteration."""
import ctypes as C
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import deep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _view(fr, cx="-0.5", cy="0", frac_bits=0, reserved=0):
    return fr._capi.fr_deep_view(cx.encode() if isinstance(cx, str) else cx, cy.encode() if isinstance(cy, str) else cy,
                                 frac_bits, reserved)


def _parse(fr, s, F):
    """fr_deep_parse_fixed as a Python int (two's complement of its limbs), or the status"""
    out = (C.c_uint64 * 80)()
    n = fr.lib().fr_deep_parse_fixed(s.encode() if isinstance(s, str) else s, F, out, 80)
    if n < 0:
        return n
    v = sum(int(out[i]) << (64 * i) for i in range(n))
    return v - (1 << (64 * n)) if v >> (64 * n - 1) else v


# ---- ABI -----------------------------------------------------------------------------------------------------------
def test_deep_view_layout_and_default(fr, tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("gcc not available")
    mirror = fr._capi.fr_deep_view
    lines = ['printf("sizeof %zu\\n", sizeof(fr_deep_view));']
    for fname, _ in mirror._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(fr_deep_view, {fname}));')
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"fractalrenderer_amd.h\"\n"
                   "#if !defined(FR_HAS_DEEP) || FR_HAS_DEEP != 1\n#error FR_HAS_DEEP\n#endif\n"
                   "int main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n") if line)
    assert int(got["sizeof"]) == C.sizeof(mirror) == 24
    for fname, _ in mirror._fields_:
        assert int(got[fname]) == getattr(mirror, fname).offset, fname
    assert C.sizeof(fr._capi.fr_params) == 112

    v = _view(fr, "9", "9", 7, 7)
    assert fr.lib().fr_deep_view_default(C.byref(v)) == 0
    assert (v.center_x, v.center_y, v.frac_bits, v.reserved) == (b"-0.5", b"0", 0, 0)
    assert fr.lib().fr_deep_view_default(None) == fr._capi.FR_ERR_INVALID_ARG
    d = fr.DeepView()
    assert (d.center_x, d.center_y, d.frac_bits) == ("-0.5", "0", 0)


def test_frac_bits_follow_the_formula(fr):
    zooms = [10.0 ** -e for e in range(13, 291)] + [3.0, 1e3, 1.5, 0.1, 7.3e-57, 2.2e-200]
    for z in zooms:
        assert fr.lib().fr_deep_frac_bits(z) == R.frac_bits(z) == fr.deep_frac_bits(z), z
    assert R.frac_bits(1e-13) == 192 and R.frac_bits(1e-290) == 1152 and R.frac_bits(3.0) == 128
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert fr.lib().fr_deep_frac_bits(bad) == fr._capi.FR_ERR_INVALID_ARG


# ---- parser ----------------------------------------------------------------------------------------------------------
def test_parser_known_answers(fr):
    F = 128
    q, r = divmod(1 << 128, 10)
    assert _parse(fr, "0.1", F) == q + (1 if 2 * r > 10 or (2 * r == 10 and q & 1) else 0)
    cases = ["0.1", "-0.1", "+0.1", "1e-3", "1E-3", "-2.5E+2", "2.5e2", "0.000123e-7", "-0", "0", "0.0e0", "3",
             "12345678.5e-1", "1" + "0" * 40 + "e-45", "0.5e-1234", "7e-1300", "-4294967295.9999", "1.5", "-1.5", "2.5",
             "0." + "0" * 37 + "5", "0." + "0" * 37 + "15", "-0." + "0" * 37 + "25", "9" * 300 + "e-300",
             R.VIEW_A["cx"], R.VIEW_A["cy"], R.VIEW_B["cx"], R.VIEW_B["cy"]]
    for F in (128, 130, 191, 192, 1152, 4096):
        for s in cases:
            assert _parse(fr, s, F) == R.parse_fixed(s, F), (s, F)
    # ties to even at the last fraction bit: 2^-129 = 0.5 ulp rounds to 0, 3 * 2^-129 = 1.5 ulp to 2 ulp
    assert _parse(fr, "1e0", 128) == 1 << 128
    for k, want in ((1, 0), (3, 2), (5, 2), (7, 4)):
        s = _exact_decimal(Fraction(k, 1 << 129))
        assert _parse(fr, s, 128) == want == R.parse_fixed(s, 128), k
        assert _parse(fr, "-" + s, 128) == -want


def _exact_decimal(q):
    """the exact decimal expansion of a dyadic rational"""
    from decimal import Decimal, getcontext
    getcontext().prec = 400
    return format(Decimal(q.numerator) / Decimal(q.denominator), "f")


def test_parser_rejects_malformed_strings(fr):
    bad = ["", "1e", "--1", "nan", "inf", "0x1p3", ".5", "5.", "1.e3", "1e+", "1 ", " 1", "1,5", "+-1", "1e3.5", "e5",
           "1" * 4097, "0." + "1" * 4095]
    for s in bad:
        assert _parse(fr, s, 128) == fr._capi.FR_ERR_INVALID_ARG, s
    assert _parse(fr, "1" * 4096, 128) == fr._capi.FR_ERR_INVALID_ARG      # well formed, but |c| >= 2^32
    assert _parse(fr, "0." + "1" * 4094, 128) == R.parse_fixed("0." + "1" * 4094, 128)   # 4096 characters: accepted
    assert _parse(fr, "4294967296", 128) == fr._capi.FR_ERR_INVALID_ARG
    assert _parse(fr, "-4294967295.99", 128) == R.parse_fixed("-4294967295.99", 128)


# ---- reference orbit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shallow", "A", "B"])
def test_reference_orbit_is_bitwise_the_python_int_orbit(fr, name):
    v = R.VIEWS[name]
    got = fr.deep_reference_orbit(fr.DeepView(v["cx"], v["cy"]), v["zoom"], v["max_iter"])
    want = R.reference_orbit(v["cx"], v["cy"], v["zoom"], v["max_iter"])
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    if name == "A":
        assert len(got) - 1 < v["max_iter"]           # this reference escapes: the m == N rebase is exercised


def test_reference_orbit_explicit_bits_and_bailout(fr):
    for cx, cy, zoom, it, bail, F in [("-0.75", "0.1", 1e-5, 300, 2.0, 130), ("0.3", "0.5", 1.0, 50, 100.0, 256),
                                      ("-1.25066", "0.02012", 1e-20, 500, 4.0, 0), ("0.25", "0", 1e-3, 200, 0.5, 128)]:
        got = fr.deep_reference_orbit(fr.DeepView(cx, cy, F), zoom, it, bail)
        want = R.reference_orbit(cx, cy, zoom, it, bail, F)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (cx, cy, F)


# ---- validation ------------------------------------------------------------------------------------------------------
def test_validation(fr):
    F = fr._capi
    L = fr.lib()
    st = fr.FractalState(zoom=1e-30)
    base = st.to_params(fr.FractalType.Mandelbrot, fr.Precision.F64)
    good = _view(fr, R.VIEW_A["cx"], R.VIEW_A["cy"])
    buf = np.empty((1001, 2), np.float64)
    n = C.c_int32()

    def orbit(v, zoom=1e-30, it=1000, bail=4.0):
        return L.fr_deep_reference_orbit(C.byref(v), zoom, it, bail, buf.ctypes.data, C.byref(n))

    assert orbit(good) == F.FR_OK
    # the view
    for s in ("", "1e", "--1", "nan", "0x1p3", "1" * 4097):
        assert orbit(_view(fr, s, "0")) == F.FR_ERR_INVALID_ARG, s
        assert orbit(_view(fr, "0", s)) == F.FR_ERR_INVALID_ARG, s
    assert orbit(_view(fr, None, "0")) == F.FR_ERR_INVALID_ARG
    assert orbit(_view(fr, "0", "0", 0, 1)) == F.FR_ERR_INVALID_ARG
    for bits in (1, 64, 127, 4097, -128):
        assert orbit(_view(fr, "0", "0", bits)) == F.FR_ERR_INVALID_ARG, bits
    for bits in (128, 129, 4096):
        assert orbit(_view(fr, "0", "0", bits)) == F.FR_OK, bits
    # zoom, max_iter, bailout
    for z in (1e-291, 0.0, -1e-30, 1001.0, float("inf"), float("nan")):
        assert orbit(good, zoom=z) == F.FR_ERR_INVALID_ARG, z
    assert orbit(good, zoom=1e-290) == F.FR_OK and orbit(good, zoom=1e3) == F.FR_OK
    for it in (0, -1, (1 << 24) + 1):
        assert orbit(good, it=it) == F.FR_ERR_INVALID_ARG, it
    for b in (0.0, -1.0, 65537.0, float("inf"), float("nan")):
        assert orbit(good, bail=b) == F.FR_ERR_INVALID_ARG, b
    assert orbit(good, bail=65536.0) == F.FR_OK
    assert L.fr_deep_reference_orbit(None, 1e-30, 100, 4.0, buf.ctypes.data, C.byref(n)) == F.FR_ERR_INVALID_ARG
    assert L.fr_deep_reference_orbit(C.byref(good), 1e-30, 100, 4.0, None, C.byref(n)) == F.FR_ERR_INVALID_ARG

    # the render entry points: a NULL context, params or view is an invalid argument
    o = F.fr_output(None, None, None, F.FR_MEM_HOST, 0)
    assert L.fr_render_deep(None, C.byref(base), C.byref(good), 64, 48, None, C.byref(o)) == F.FR_ERR_INVALID_ARG
    assert L.fr_render_deep_async(None, C.byref(base), C.byref(good), 64, 48, None, C.byref(o), None) == F.FR_ERR_INVALID_ARG


def test_validation_of_params(fr):
    """fr_deep_validate's verdicts, through the internal entry the render entry points call after their NULL checks"""
    F = fr._capi
    L = fr.lib()
    L.fr_deep_validate.restype = C.c_int
    L.fr_deep_validate.argtypes = [C.POINTER(F.fr_params), C.POINTER(F.fr_deep_view), C.c_uint32, C.c_uint32]
    good = _view(fr, R.VIEW_A["cx"], R.VIEW_A["cy"])

    def check(W=64, H=48, view=good, **kw):
        p = fr.FractalState(zoom=1e-30).to_params(fr.FractalType.Mandelbrot, fr.Precision.F64)
        for k, val in kw.items():
            setattr(p, k, val)
        return L.fr_deep_validate(C.byref(p), C.byref(view), W, H)

    assert check() == F.FR_OK
    # fractal and precision
    for t in (1, 2, 3, 4, 5, 99):
        assert check(fractal_type=t) == F.FR_ERR_UNSUPPORTED, t
    assert check(precision=0) == F.FR_ERR_UNSUPPORTED
    # effects that need the whole orbit
    assert check(orbit_trap_enabled=1) == F.FR_ERR_UNSUPPORTED
    assert check(stripe_enabled=1) == F.FR_ERR_UNSUPPORTED
    assert check(interior_style=2) == F.FR_ERR_UNSUPPORTED
    assert check(interior_style=1) == F.FR_OK
    # fr_params_validate's rules; the double centre is not read
    assert check(center_x=float("nan"), center_y=float("inf")) == F.FR_OK
    for kw in (dict(W=0), dict(H=0), dict(W=65536, H=32768), dict(max_iterations=0), dict(max_iterations=(1 << 24) + 1),
               dict(antialiasing_samples=17), dict(antialiasing_samples=-1), dict(bailout=0.0), dict(bailout=float("nan")),
               dict(bailout=65537.0), dict(zoom=1e-291), dict(zoom=1001.0), dict(zoom=-1e-30), dict(zoom=0.0),
               dict(julia_c_real=float("inf"))):
        assert check(**kw) == F.FR_ERR_INVALID_ARG, kw
    assert check(max_iterations=1 << 24, antialiasing_samples=16, bailout=65536.0) == F.FR_OK
    # the view
    assert check(view=_view(fr, "1e", "0")) == F.FR_ERR_INVALID_ARG
    assert check(view=_view(fr, "0", "0", 0, 3)) == F.FR_ERR_INVALID_ARG
    assert check(view=_view(fr, "0", "0", 100)) == F.FR_ERR_INVALID_ARG
    assert check(view=_view(fr, "1" * 4097, "0")) == F.FR_ERR_INVALID_ARG


# ---- the restatement against the direct fixed-point iteration -------------------------------------------------------
@pytest.mark.parametrize("name", ["shallow", "A", "B"])
def test_restatement_agrees_with_exact_iteration(fr, name):
    v = R.VIEWS[name]
    W, H = 256, 192
    orbit = fr.deep_reference_orbit(fr.DeepView(v["cx"], v["cy"]), v["zoom"], v["max_iter"])   # the library's orbit
    (it, _), = R.restate(v, W, H, 1, orbit=orbit)[0]
    rng = np.random.default_rng(1234)
    ys, xs = rng.integers(0, H, 256), rng.integers(0, W, 256)
    ex = np.array([R.exact_iter(v["cx"], v["cy"], int(x), int(y), W, H, v["zoom"], v["max_iter"]) for x, y in zip(xs, ys)])
    assert (ex == it[ys, xs]).mean() >= 0.99


@pytest.mark.parametrize("name", ["A", "B"])
def test_deep_views_are_what_the_tests_need(fr, name):
    """20-95 % of the samples escape, at least one rebase per 100 samples, no exact iter value covers 60 % of the sample"""
    v = R.VIEWS[name]
    W, H = 256, 192
    orbit = fr.deep_reference_orbit(fr.DeepView(v["cx"], v["cy"]), v["zoom"], v["max_iter"])
    samples, rebases = R.restate(v, W, H, 1, orbit=orbit)
    it = samples[0][0]
    assert 0.20 <= (it < v["max_iter"]).mean() <= 0.95
    assert rebases >= it.size / 100
    rng = np.random.default_rng(1234)
    ys, xs = rng.integers(0, H, 256), rng.integers(0, W, 256)
    ex = [R.exact_iter(v["cx"], v["cy"], int(x), int(y), W, H, v["zoom"], v["max_iter"]) for x, y in zip(xs, ys)]
    assert np.unique(ex, return_counts=True)[1].max() <= 0.60 * len(ex)
