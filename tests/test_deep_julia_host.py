"""Deep Julia views (fr_render_deep_julia, fr_render_deepx_julia): the parts that need no GPU -- the header macros and
exported symbols, both reference orbits bit for bit against Python integers in double and in extended storage, validation,
and, on the restatement alone, the predicates that make the GPU comparisons meaningful."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import deep_julia_ref as J
import deepx_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 256, 192


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _dv(fr, cx="0", cy="0", frac_bits=0, reserved=0):
    enc = lambda s: s.encode() if isinstance(s, str) else s
    return fr._capi.fr_deep_view(enc(cx), enc(cy), frac_bits, reserved)


def _xv(fr, cx="0", cy="0", zoom="1e-400", frac_bits=0, reserved=0):
    enc = lambda s: s.encode() if isinstance(s, str) else s
    return fr._capi.fr_deepx_view(enc(cx), enc(cy), enc(zoom), frac_bits, reserved)


# ---- ABI -----------------------------------------------------------------------------------------------------------
def test_header_macros_and_symbols(fr, tmp_path):
    for name in ("fr_deep_julia_reference_orbits", "fr_deepx_julia_reference_orbits", "fr_deep_julia_validate",
                 "fr_deepx_julia_validate", "fr_render_deep_julia", "fr_render_deep_julia_async", "fr_render_deepx_julia",
                 "fr_render_deepx_julia_async"):
        assert name in fr._capi.SIGNATURES and getattr(fr.lib(), name)
    assert callable(fr.deep_julia_reference_orbits) and callable(fr.Renderer.render_deep_julia)
    gcc = shutil.which("gcc")
    if gcc:
        src = tmp_path / "macros.c"
        src.write_text("#include \"fractalrenderer_amd.h\"\n"
                       "#if !defined(FR_HAS_DEEP_JULIA) || FR_HAS_DEEP_JULIA != 1\n#error FR_HAS_DEEP_JULIA\n#endif\n"
                       "#if !defined(FR_HAS_DEEPX_JULIA) || FR_HAS_DEEPX_JULIA != 1\n#error FR_HAS_DEEPX_JULIA\n#endif\n"
                       "int (*a)(const fr_deep_view*, double, double, double, int32_t, float, double*, int32_t*, double*, int32_t*)"
                       " = fr_deep_julia_reference_orbits;\n"
                       "int (*b)(const fr_deepx_view*, double, double, int32_t, float, double*, int32_t*, int32_t*, double*, int32_t*,"
                       " int32_t*) = fr_deepx_julia_reference_orbits;\n"
                       "int (*c)(const fr_params*, const fr_deep_view*, uint32_t, uint32_t) = fr_deep_julia_validate;\n"
                       "int (*d)(const fr_params*, const fr_deepx_view*, uint32_t, uint32_t) = fr_deepx_julia_validate;\n"
                       "int (*e)(fr_ctx*, const fr_params*, const fr_deep_view*, uint32_t, uint32_t, const fr_shard*, const fr_output*)"
                       " = fr_render_deep_julia;\n"
                       "int (*f)(fr_ctx*, const fr_params*, const fr_deep_view*, uint32_t, uint32_t, const fr_shard*, const fr_output*,"
                       " void*) = fr_render_deep_julia_async;\n"
                       "int (*g)(fr_ctx*, const fr_params*, const fr_deepx_view*, uint32_t, uint32_t, const fr_shard*, const fr_output*)"
                       " = fr_render_deepx_julia;\n"
                       "int (*h)(fr_ctx*, const fr_params*, const fr_deepx_view*, uint32_t, uint32_t, const fr_shard*, const fr_output*,"
                       " void*) = fr_render_deepx_julia_async;\n")
        subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "macros.o")], check=True)


# ---- the reference orbits ------------------------------------------------------------------------------------------------
def test_the_centres_are_the_fixed_points():
    """the leading digits the issue gives, for comparison only: the strings come from decimal at 1300 digits"""
    lead = {"RABBIT30": ("-0.27373934618672526", "0.47819721437651755"), "DENDRITE30": ("-0.30024259022012041", "0.62481053384382658"),
            "DUST30": ("-0.52750311864353463", "0.07591217835228786"), "BASILICA30": ("-0.61803398874989484", "0")}
    for name, (lx, ly) in lead.items():
        v = J.view(name)
        assert v["cx"].startswith(lx) and v["cy"].startswith(ly), (name, v["cx"], v["cy"])
        assert len(v["cx"].split(".")[1]) == 45
    assert J.view("BASILICA30")["cy"] == "0"
    assert len(J.view("DENDRITE100")["cx"].split(".")[1]) == 115 and J.view("DENDRITE100")["cx"].startswith(J.view("DENDRITE30")["cx"][:40])


@pytest.mark.parametrize("name", ["RABBIT30", "DUST30", "DENDRITE100"])
def test_both_orbits_match_python_integers(fr, name):
    v = J.view(name)
    P, Q = J.reference_orbits(v)
    gP, gQ = fr.deep_julia_reference_orbits(fr.DeepView(v["cx"], v["cy"]), v["c"], v["max_iter"], zoom=v["zoom"])
    assert fr.deep_frac_bits(v["zoom"]) == v["F"]
    assert _bits(gP, P) and _bits(gQ, Q)
    (Pm, Pe), (Qm, Qe) = J.reference_orbits_x(v)
    (gPm, gPe), (gQm, gQe) = fr.deep_julia_reference_orbits(fr.DeepView(v["cx"], v["cy"], zoom=v["zoom_s"]), v["c"], v["max_iter"])
    assert _bits(gPm, Pm) and _bits(gPe, Pe) and _bits(gQm, Qm) and _bits(gQe, Qe)
    assert Qe[0] == X.X_ZERO and Pe[0] == 0 and np.all(Qm[1] == np.array(v["c"]))          # Q_0 = 0, Q_1 = c
    # Q is fr_deep_reference_orbit's orbit at C = c
    cs = [format(J.decimal.Decimal(x), "f") for x in v["c"]]
    assert _bits(fr.deep_reference_orbit(fr.DeepView(cs[0], cs[1], v["F"]), v["zoom"], v["max_iter"]), Q)
    want = {"RABBIT30": (1072, 1100), "DUST30": (1600, 253), "DENDRITE100": (817, 1200)}[name]
    assert (len(P) - 1, len(Q) - 1) == want


def test_c_enters_the_fixed_point_exactly_or_rounded_to_even(fr):
    """a c that F = 128 cannot hold: round_half_even(c 2^F), as Python's round(Fraction) has it"""
    for c in ((2.0 ** -129, -2.0 ** -129), (3 * 2.0 ** -130, 2.0 ** -1074), (-(2.0 ** -128 + 2.0 ** -180), 0.3)):
        v = dict(c=c, cx="0.25", cy="-0.125", zoom=1.0, max_iter=12, F=128)
        P, Q = J.reference_orbits(v)
        gP, gQ = fr.deep_julia_reference_orbits(fr.DeepView(v["cx"], v["cy"], 128), c, 12, zoom=1.0)
        assert _bits(gP, P) and _bits(gQ, Q), c


# ---- validation ---------------------------------------------------------------------------------------------------------
def test_validation_with_no_device(fr):
    L, K = fr.lib(), fr._capi
    E, U = K.FR_ERR_INVALID_ARG, K.FR_ERR_UNSUPPORTED
    julia, f64 = fr.FractalType.JuliaSet, fr.Precision.F64
    st = lambda **kw: fr.FractalState(max_iterations=64, **kw)
    for check, view in ((lambda p, v, w=8, h=8: L.fr_deep_julia_validate(C.byref(p), C.byref(v), w, h), _dv),
                        (lambda p, v, w=8, h=8: L.fr_deepx_julia_validate(C.byref(p), C.byref(v), w, h), _xv)):
        ok = st(zoom=1e-30).to_params(julia, f64, False)
        assert check(ok, view(fr)) == 0
        assert check(st(zoom=1e-30, center_x=1e30, center_y=-1e30).to_params(julia, f64, False), view(fr)) == 0
        for flag in (K.FR_FLAG_DEEP_BLA, K.FR_FLAG_DEEPX_BLA, K.FR_FLAG_DEEP_SHIP_BLA, K.FR_FLAG_DEEPX_SHIP_BLA):
            p = st().to_params(julia, f64, False)
            p.flags |= flag
            assert check(p, view(fr)) == U, flag
        for other in (fr.FractalType.Mandelbrot, fr.FractalType.BurningShip):
            assert check(st().to_params(other, f64, False), view(fr)) == U
        assert check(st().to_params(julia, fr.Precision.F32, False), view(fr)) == U
        # Julia has no trap, stripe or interior styles: ignored, as fr_render ignores them
        assert check(st(orbit_trap_enabled=True, stripe_enabled=True, interior_style=2).to_params(julia, f64, False), view(fr)) == 0
        assert check(st(bailout=1e6).to_params(julia, f64, False), view(fr)) == E
        assert check(st(bailout=65536.0).to_params(julia, f64, False), view(fr)) == 0
        for c in ((float("nan"), 0.0), (0.0, float("inf")), (2.0 ** 32, 0.0), (0.0, -(2.0 ** 32))):
            assert check(st(julia_c_real=c[0], julia_c_imag=c[1]).to_params(julia, f64, False), view(fr)) == E, c
        assert check(st(julia_c_real=2.0 ** 32 - 1.0, julia_c_imag=-3.5).to_params(julia, f64, False), view(fr)) == 0
        # the centre rule: |P_0|^2 > bailout^2, compared exactly
        assert check(ok, view(fr, cx="4", cy="0")) == 0
        assert check(ok, view(fr, cx="4", cy="1e-30")) == E
        assert check(ok, view(fr, cx="-3", cy="3")) == E
        assert check(st(bailout=0.5).to_params(julia, f64, False), view(fr, cx="0.3", cy="0.4")) == 0
        assert check(st(bailout=0.5).to_params(julia, f64, False), view(fr, cx="0.3", cy="0.4000000000000000000000000001")) == E
        assert check(ok, view(fr, frac_bits=100)) == E and check(ok, view(fr, reserved=1)) == E
        assert check(ok, view(fr, cx="1e")) == E and check(ok, view(fr, cy=None)) == E
        assert check(ok, view(fr), 0, 8) == E
    xcheck = lambda p, v: L.fr_deepx_julia_validate(C.byref(p), C.byref(v), 8, 8)
    ok = st().to_params(julia, f64, False)
    assert xcheck(st(zoom=1e30).to_params(julia, f64, False), _xv(fr)) == 0           # p->zoom is ignored there
    for z in ("1e-1001", "2e3", "z", "", "0", "-1", None):
        assert xcheck(ok, _xv(fr, zoom=z)) == E, z
    assert xcheck(ok, _xv(fr, zoom="1e-1000")) == 0 and xcheck(ok, _xv(fr, zoom="1e3")) == 0
    assert L.fr_deep_julia_validate(C.byref(st(zoom=1e-291).to_params(julia, f64, False)), C.byref(_dv(fr)), 8, 8) == E
    assert L.fr_deep_julia_validate(None, C.byref(_dv(fr)), 8, 8) == E and L.fr_deepx_julia_validate(C.byref(ok), None, 8, 8) == E
    # the other deep families keep rejecting Julia
    assert L.fr_deep_validate(C.byref(ok), C.byref(_dv(fr)), 8, 8) == U
    assert L.fr_deep_ship_validate(C.byref(ok), C.byref(_dv(fr)), 8, 8) == U
    assert L.fr_deepx_validate(C.byref(ok), C.byref(_xv(fr)), 8, 8) == U
    assert L.fr_deepx_ship_validate(C.byref(ok), C.byref(_xv(fr)), 8, 8) == U
    # the orbit entries: their own argument checks
    a = np.empty((9, 2)); b = np.empty((9, 2)); ea = np.empty(9, np.int32); eb = np.empty(9, np.int32)
    na, nb = C.c_int32(), C.c_int32()
    f = lambda v=_dv(fr), cr=-0.12, ci=0.74, zoom=1e-30, n=8, bail=4.0, pa=a.ctypes.data, pb=b.ctypes.data: \
        L.fr_deep_julia_reference_orbits(C.byref(v) if v else None, cr, ci, zoom, n, C.c_float(bail), pa, C.byref(na), pb, C.byref(nb))
    assert f() == 0 and na.value == 9 and nb.value == 9
    assert f(n=0) == E and f(bail=0.0) == E and f(cr=float("nan")) == E and f(ci=2.0 ** 32) == E and f(zoom=1e-300) == E
    assert f(pa=None) == E and f(pb=None) == E and f(v=None) == E and f(v=_dv(fr, cx="5")) == E
    g = lambda v=_xv(fr), cr=-0.12, n=8, pa=a.ctypes.data, pe=ea.ctypes.data: \
        L.fr_deepx_julia_reference_orbits(C.byref(v) if v else None, cr, 0.74, n, C.c_float(4.0), pa, pe, C.byref(na), b.ctypes.data,
                                          eb.ctypes.data, C.byref(nb))
    assert g() == 0 and na.value == 9 and nb.value == 9 and eb[0] == X.X_ZERO
    assert g(n=0) == E and g(cr=float("inf")) == E and g(pa=None) == E and g(pe=None) == E and g(v=None) == E
    assert g(v=_xv(fr, zoom="1e-2000")) == E and g(v=_xv(fr, cx="-5")) == E
    # the render entries check their arguments before they touch a device: ctx NULL comes first
    o = K.fr_output(None, None, None, K.FR_MEM_HOST, 0)
    dv, xv = _dv(fr), _xv(fr)
    assert L.fr_render_deep_julia(None, C.byref(ok), C.byref(dv), 8, 8, None, C.byref(o)) == E
    assert L.fr_render_deep_julia_async(None, C.byref(ok), C.byref(dv), 8, 8, None, C.byref(o), None) == E
    assert L.fr_render_deepx_julia(None, C.byref(ok), C.byref(xv), 8, 8, None, C.byref(o)) == E
    assert L.fr_render_deepx_julia_async(None, C.byref(ok), C.byref(xv), 8, 8, None, C.byref(o), None) == E


# ---- the restatement: what makes the GPU comparisons meaningful ------------------------------------------------------------
@pytest.mark.parametrize("name", ["RABBIT30", "DENDRITE100", "DUST30"])
def test_the_views_exercise_what_they_are_for(name):
    v = J.view(name)
    samples, stats = J.restated(name)
    it = samples[0][0]
    P, Q = J.reference_orbits(v)
    print(name, "escaped", (it < v["max_iter"]).mean(), "distinct", len(np.unique(it)), stats, "N_P", len(P) - 1, "N_Q", len(Q) - 1)
    assert (it < v["max_iter"]).mean() >= 0.10
    assert len(np.unique(it)) >= 30
    assert stats["moved"][0] >= 0.5
    if name == "DUST30":
        assert len(Q) - 1 < v["max_iter"]                          # Q ends: rebases by m == N_Q
    else:
        assert len(P) - 1 < v["max_iter"]                          # P ends before max_iter
    ex = J.exact_samples(name)
    ys, xs = J.random_pixels(W, H)
    largest = np.unique(ex, return_counts=True)[1].max() / len(ex)
    agreement = (it[ys, xs] == ex).mean()
    print("largest exact class", largest, "agreement", agreement)
    assert largest <= 0.80 and agreement >= 0.99


def test_dendrite30_orbit_ends_before_max_iter():
    v = J.view("DENDRITE30")
    P, Q = J.reference_orbits(v)
    assert (len(P) - 1, len(Q) - 1) == (321, 400)


@pytest.mark.parametrize("name", ["RABBIT30", "BASILICA30"])
def test_extended_restatement_equals_the_fp64_one_on_views_a_double_holds(name):
    a = J.restate(J.view(name), 64, 48)
    stats = {}
    b = J.restate_x(J.view(name), 64, 48, stats=stats)
    assert np.array_equal(a[0][0], b[0][0]) and _bits(a[0][1], b[0][1])
    print(name, stats)
    if name == "BASILICA30":                                       # superattracting interior: the flush fires
        assert stats["flushes"] > 0 and stats["ext_steps"] > 0


@pytest.mark.parametrize("name", ["DENDRITE400", "DENDRITE1000"])
def test_extended_restatement_agrees_with_the_exact_iteration(name):
    v = J.view(name)
    assert X.frac_bits_x(v["zoom_s"]) == v["F"]
    assert X.zoom_pair(v["zoom_s"]) == {"DENDRITE400": (1.1718289888396993, -1329), "DENDRITE1000": (1.0511037747648835, -3322)}[name]
    samples, stats = J.restated_x(name)
    it = samples[0][0]
    ex = J.exact_samples_x(name)
    ys, xs = J.random_pixels(J.XW, J.XH)
    largest = np.unique(ex, return_counts=True)[1].max() / len(ex)
    print(name, stats, "exact", ex.min(), ex.max(), "largest class", largest, "agreement", (it[ys, xs] == ex).mean())
    assert largest <= 0.80 and (it[ys, xs] == ex).mean() >= 0.99
    assert stats["ext_steps"] > stats["plain_steps"]


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_shallow_views_agree_with_the_direct_fp64_iteration(k):
    v = J.SHALLOW[k]
    it = J.restated(str(k))[0][0][0]
    direct = J.direct_fp64(v, W, H)
    print(v["name"], "agreement", (it == direct).mean())
    assert (it == direct).mean() >= 0.98
    if k == 0:                                                     # centre 0: P equals Q
        P, Q = J.reference_orbits(v)
        assert _bits(P, Q)
