"""Deep views with extended-exponent deltas (fr_render_deepx): the parts that need no GPU -- ABI layout and defaults, the
zoom string as a (mantissa, exponent) pair against Fraction, the automatic fraction bits, validation, the reference
orbit in the extended storage against Python integers, and the numpy restatement of the two-mode step against the plain
restatement (shallow views, bit for bit) and against the direct fixed-point iteration (deep views)."""
import ctypes as C
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import deep_ref as R
import deepx_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 256, 192
V = X.views()


def _view(fr, cx="-0.5", cy="0", zoom="3", frac_bits=0, reserved=0):
    enc = lambda s: s.encode() if isinstance(s, str) else s
    return fr._capi.fr_deepx_view(enc(cx), enc(cy), enc(zoom), frac_bits, reserved)


def _zoom(fr, s):
    zm, ze = C.c_double(-1.0), C.c_int32(-1)
    st = fr.lib().fr_deepx_zoom(s.encode() if isinstance(s, str) else s, C.byref(zm), C.byref(ze))
    return st if st else (zm.value, ze.value)


def _orbit(fr, v, max_iter, bailout=4.0):
    mant = np.empty((max_iter + 1, 2), np.float64)
    exp2 = np.empty(max_iter + 1, np.int32)
    n = C.c_int32()
    st = fr.lib().fr_deepx_reference_orbit(C.byref(v), max_iter, C.c_float(bailout), mant.ctypes.data, exp2.ctypes.data,
                                           C.byref(n))
    return st if st else (mant[:n.value].copy(), exp2[:n.value].copy())


# ---- ABI -----------------------------------------------------------------------------------------------------------
def test_deepx_view_layout_symbols_and_default(fr, tmp_path):
    mirror = fr._capi.fr_deepx_view
    assert C.sizeof(mirror) == 32 and C.sizeof(fr._capi.fr_deep_view) == 24 and C.sizeof(fr._capi.fr_params) == 112
    for name in ("fr_deepx_view_default", "fr_deepx_zoom", "fr_deepx_frac_bits", "fr_deepx_reference_orbit", "fr_render_deepx",
                 "fr_render_deepx_async"):
        assert name in fr._capi.SIGNATURES and getattr(fr.lib(), name)
    gcc = shutil.which("gcc")
    if gcc:
        lines = ['printf("sizeof %zu\\n", sizeof(fr_deepx_view));', 'printf("zero %d\\n", FR_DEEPX_ZERO_EXP);']
        for fname, _ in mirror._fields_:
            lines.append(f'printf("{fname} %zu\\n", offsetof(fr_deepx_view, {fname}));')
        src = tmp_path / "layout.c"
        src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"fractalrenderer_amd.h\"\n"
                       "#if !defined(FR_HAS_DEEPX) || FR_HAS_DEEPX != 1\n#error FR_HAS_DEEPX\n#endif\n"
                       "int main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n")
        exe = tmp_path / "layout"
        subprocess.run([gcc, "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        got = dict(line.split() for line in
                   subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n") if line)
        assert int(got["sizeof"]) == 32 and int(got["zero"]) == X.X_ZERO
        for fname, _ in mirror._fields_:
            assert int(got[fname]) == getattr(mirror, fname).offset, fname
    v = _view(fr, "9", "9", "9", 7, 7)
    assert fr.lib().fr_deepx_view_default(C.byref(v)) == 0
    assert (v.center_x, v.center_y, v.zoom, v.frac_bits, v.reserved) == (b"-0.5", b"0", b"3", 0, 0)
    assert fr.lib().fr_deepx_view_default(None) == fr._capi.FR_ERR_INVALID_ARG
    assert fr.DeepView().zoom is None and fr.DeepView(zoom="1e-400").to_cx().zoom == b"1e-400"


# ---- the zoom ---------------------------------------------------------------------------------------------------------
ZOOMS = ["3", "1e3", "1000", "1E+3", "0.5", "1", "1e-30", "1e-100", "1e-290", "1e-300", "2.2250738585072014e-308",
         "2.2250738585072009e-308", "1e-310", "4.9e-324", "2.4703282292062327e-324", "1e-330", "1e-400", "1e-1000",
         "1.0e-999", "9.99999999999999999999e-1000", "0." + "0" * 999 + "1", "123456789012345678901234567890e-500",
         # ties at the 53rd bit: 1 + 2^-53 exactly (to even: down), a hair above (up), 1 + 3 2^-53 (to even: up)
         "1.00000000000000011102230246251565404236316680908203125",
         "1.00000000000000011102230246251565404236316680908203125" + "0" * 40 + "1",
         "1.00000000000000033306690738754696212708950042724609375",
         "9007199254740993e-20", "9007199254740993", "0.1", "7e-777", "3." + "3" * 2000]


@pytest.mark.parametrize("s", ZOOMS, ids=[z[:24] for z in ZOOMS])
def test_zoom_pair_is_correctly_rounded(fr, s):
    if Fraction(s) > 1000:
        assert _zoom(fr, s) == fr._capi.FR_ERR_INVALID_ARG
        return
    zm, ze = _zoom(fr, s)
    assert (zm, ze) == X.zoom_pair(s) and 1.0 <= zm < 2.0
    assert fr.deepx_zoom(s) == (zm, ze)
    # half an ulp of the 53-bit mantissa bounds the error
    assert abs(Fraction(zm) * Fraction(2) ** ze - Fraction(s)) <= Fraction(2) ** (ze - 53)


def test_zoom_range_and_grammar(fr):
    E = fr._capi.FR_ERR_INVALID_ARG
    for bad in ("9.9e-1001", "1e-1001", "1e-5000", "1e-999999999", "1000.0000001", "1.1e3", "1e4", "1e999999999", "0", "0.0",
                "-1", "-1e-400", "", "abc", "1e", "1.", ".5", "1e-400 ", " 1", "1e-4.5", "0x1p-3", "nan", "inf",
                "1" * 4097):
        assert _zoom(fr, bad) == E, bad
        assert fr.lib().fr_deepx_frac_bits(bad.encode()) == E, bad
    assert fr.lib().fr_deepx_zoom(None, C.byref(C.c_double()), C.byref(C.c_int32())) == E
    assert fr.lib().fr_deepx_zoom(b"1", None, None) == E
    assert fr.lib().fr_deepx_frac_bits(None) == E
    assert _zoom(fr, "+1e-1000") == X.zoom_pair("1e-1000") == (1.0511037747648835, -3322)
    assert _zoom(fr, "1e3") == (1.953125, 9)


def test_frac_bits_follow_fr_deep_frac_bits_and_the_rule_beyond(fr):
    rng = np.random.default_rng(5)
    doubles = [3.0, 1e3, 1.0, 1e-30, 1e-100, 1e-290, 1.0000000000000002e-290, 4.2e-150]
    doubles += [float(10.0 ** -e * m) for e, m in zip(rng.uniform(0, 289, 200), rng.uniform(1, 10, 200))]
    for d in doubles:
        assert fr.lib().fr_deepx_frac_bits(repr(d).encode()) == fr.lib().fr_deep_frac_bits(d) == R.frac_bits(d), d
    for s, want in (("1e-400", 1472), ("1e-1000", 3456), ("1e-100", 512)):
        assert fr.lib().fr_deepx_frac_bits(s.encode()) == want == X.frac_bits_x(s)
    for s in ("1e-291", "1e-300", "1e-308", "1e-320", "5e-324", "1e-330", "3.3e-555", "7e-777", "2e-999"):
        got = fr.lib().fr_deepx_frac_bits(s.encode())
        assert got == X.frac_bits_x(s) == fr.deepx_frac_bits(s)
        bits = 128 + int(-(math.log10(X.zoom_pair(s)[0]) + X.zoom_pair(s)[1] * math.log10(2.0)) * 3.32)
        assert got == (bits + 63) // 64 * 64 and got % 64 == 0 and 1024 <= got <= 3456


# ---- validation ---------------------------------------------------------------------------------------------------------
def test_validation_of_every_rejected_input(fr):
    L = fr.lib()
    E, U = fr._capi.FR_ERR_INVALID_ARG, fr._capi.FR_ERR_UNSUPPORTED
    mant = np.empty((9, 2)); exp2 = np.empty(9, np.int32); n = C.c_int32()

    def orbit(v, max_iter=8, bailout=4.0):
        return L.fr_deepx_reference_orbit(C.byref(v), max_iter, C.c_float(bailout), mant.ctypes.data, exp2.ctypes.data, C.byref(n))

    assert orbit(_view(fr)) == 0 and n.value >= 2
    assert orbit(_view(fr, reserved=1)) == E
    for fb in (-1, 1, 127, 4097):
        assert orbit(_view(fr, frac_bits=fb)) == E, fb
    assert orbit(_view(fr, frac_bits=128)) == 0 and orbit(_view(fr, frac_bits=4096)) == 0
    for z in ("1e-1001", "1e4", "0", "-3", "x", ""):
        assert orbit(_view(fr, zoom=z)) == E, z
    assert orbit(_view(fr, zoom=None)) == E and orbit(_view(fr, cx=None)) == E and orbit(_view(fr, cy=None)) == E
    assert orbit(_view(fr, cx="1e")) == E and orbit(_view(fr, cy="5e9")) == E
    assert orbit(_view(fr), max_iter=0) == E and orbit(_view(fr), max_iter=(1 << 24) + 1) == E
    assert orbit(_view(fr), bailout=0.0) == E and orbit(_view(fr), bailout=1e6) == E
    assert L.fr_deepx_reference_orbit(None, 8, C.c_float(4.0), mant.ctypes.data, exp2.ctypes.data, C.byref(n)) == E
    v = _view(fr)
    assert L.fr_deepx_reference_orbit(C.byref(v), 8, C.c_float(4.0), None, exp2.ctypes.data, C.byref(n)) == E
    assert L.fr_deepx_reference_orbit(C.byref(v), 8, C.c_float(4.0), mant.ctypes.data, None, C.byref(n)) == E
    assert L.fr_deepx_reference_orbit(C.byref(v), 8, C.c_float(4.0), mant.ctypes.data, exp2.ctypes.data, None) == E
    # the render entries check their arguments before they touch a device: ctx NULL comes first
    p = fr.FractalState().to_params(fr.FractalType.Mandelbrot, fr.Precision.F64, False)
    o = fr._capi.fr_output(None, None, None, fr._capi.FR_MEM_HOST, 0)
    assert L.fr_render_deepx(None, C.byref(p), C.byref(v), 8, 8, None, C.byref(o)) == E
    assert L.fr_render_deepx_async(None, C.byref(p), C.byref(v), 8, 8, None, C.byref(o), None) == E
    assert U != E


# ---- the reference orbit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["T110", "T280", "T320", "D", "E"])
def test_orbit_matches_python_integers_and_decodes_to_the_doubles(fr, name):
    v = V[name]
    n = min(v["max_iter"], 1200)                                   # E: 1200 steps of 3456-bit Python integers are enough
    got = _orbit(fr, _view(fr, v["cx"], v["cy"], v["zoom"]), n)
    F = X.frac_bits_x(v["zoom"])
    mant, exp2 = X.reference_orbit_x(v["cx"], v["cy"], F, n)
    assert np.array_equal(got[0].view(np.uint64), mant.view(np.uint64)) and np.array_equal(got[1], exp2)
    assert exp2[0] == X.X_ZERO and np.all(exp2[1:] == 0)           # a dendrite's orbit stays of order 1
    # the same F through fr_deep_reference_orbit (its zoom only selects F): the same doubles
    old = np.empty((n + 1, 2)); ln = C.c_int32()
    dv = fr._capi.fr_deep_view(v["cx"].encode(), v["cy"].encode(), F, 0)
    assert fr.lib().fr_deep_reference_orbit(C.byref(dv), 1e-100, n, C.c_float(4.0), old.ctypes.data, C.byref(ln)) == 0
    assert ln.value == len(exp2)
    assert np.array_equal(X.decode(*got).view(np.uint64), old[:ln.value].view(np.uint64))
    m2, e2 = fr.deepx_reference_orbit(fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"]), n)
    assert np.array_equal(m2, mant) and np.array_equal(e2, exp2)


def test_shallow_views_get_the_orbit_of_fr_render_deep(fr):
    for name in ("A", "B", "shallow"):
        v = R.VIEWS[name]
        mant, exp2 = _orbit(fr, _view(fr, v["cx"], v["cy"], repr(v["zoom"])), v["max_iter"])
        want = R.reference_orbit(v["cx"], v["cy"], v["zoom"], v["max_iter"])
        assert np.array_equal(X.decode(mant, exp2).view(np.uint64), want.view(np.uint64)), name


def test_nucleus_orbit_keeps_what_a_double_flushes(fr):
    """centred on the period-201 nucleus (420 of its digits): Z_201, Z_402, ... return far below the double range"""
    c = V["nucleus201"]
    zoom, n = "1e-300", 450
    F = X.frac_bits_x(zoom)
    ints = X.fixed_orbit(c["cx"], c["cy"], F, n)
    assert len(ints) == n + 1
    for k in (201, 402):
        assert 0 < max(abs(ints[k][0]), abs(ints[k][1])) < 1 << (F - 1040), k     # |Z_k| < 2^-1040 (about 1e-313)
    mant, exp2 = _orbit(fr, _view(fr, c["cx"], c["cy"], zoom), n)
    pm, pe = X.reference_orbit_x(c["cx"], c["cy"], F, n)
    assert np.array_equal(mant.view(np.uint64), pm.view(np.uint64)) and np.array_equal(exp2, pe)
    old = np.empty((n + 1, 2)); ln = C.c_int32()
    dv = fr._capi.fr_deep_view(c["cx"].encode(), c["cy"].encode(), F, 0)
    assert fr.lib().fr_deep_reference_orbit(C.byref(dv), 1e-100, n, C.c_float(4.0), old.ctypes.data, C.byref(ln)) == 0
    for k in (201, 402):
        zr, zi = ints[k]
        e = int(exp2[k])
        assert e < -1040 and 0.5 <= np.abs(mant[k]).max() < 1.0
        assert e == max(abs(zr), abs(zi)).bit_length() - F
        for comp, z in zip(mant[k], (zr, zi)):                     # each mantissa within half an ulp of the exact value
            assert abs(Fraction(float(comp)) * Fraction(2) ** e - Fraction(z, 1 << F)) <= Fraction(2) ** (e - 53)
        assert np.all(np.abs(old[k]) < 2.0 ** -1022)              # fr_deep_reference_orbit: 0 or a subnormal
    normal = exp2 == 0
    assert normal.sum() >= n - 2
    assert np.array_equal(mant[normal].view(np.uint64), old[:n + 1][normal].view(np.uint64))


# ---- the restatement --------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_plain_one_on_shallow_views():
    """views whose dc is at least 2^-400 leave the extended mode on their first step: the planes of deep_ref.restate"""
    rows = list(range(90, 102))
    for name, aa in (("A", 1), ("B", 2), ("shallow", 1)):
        v = R.VIEWS[name]
        vx = dict(cx=v["cx"], cy=v["cy"], zoom=repr(v["zoom"]), max_iter=v["max_iter"])
        stats = {}
        got = X.restate_x(vx, W, H, aa, rows=rows, stats=stats)
        want, _ = R.restate(v, W, H, aa, rows=rows)
        for (gi, gr), (wi, wr) in zip(got, want):
            assert np.array_equal(gi, wi) and np.array_equal(gr.view(np.uint64), wr.view(np.uint64)), name
        # A, B: one extended step per sample, and the one sample with dc = 0 (aa 1, the frame's centre) that never leaves;
        # the shallow view holds c = 0, whose z = 0 is rebased onto the orbit's start at every step
        if name != "shallow":
            assert stats["ext_steps"] <= len(rows) * W * aa * aa + v["max_iter"] and stats["to_ext"] == 0, stats


def _pixels(view, xs, ys, stats=None):
    zm, ze = X.zoom_pair(view["zoom"])
    dc = X.sample_dc_x(W, H, zm, ze, 1, 0, rows=ys)
    sel = np.arange(len(ys)) * W + xs
    mant, exp2 = X.orbit_of(view)
    return X.perturb_x(mant, exp2, tuple(a[sel] for a in dc), view["max_iter"], stats=stats)[0]


@pytest.mark.parametrize("name", ["T110", "T130", "T260", "T280", "T300", "T320", "D", "E"])
def test_restatement_agrees_with_the_exact_iteration(name):
    g = X.exact_golden()
    v, ex = V[name], g[name]
    stats = {}
    it = _pixels(v, g["xs"], g["ys"], stats)
    print(name, "agreement", (it == ex).mean(), stats)
    assert np.unique(ex, return_counts=True)[1].max() <= 0.60 * len(ex)
    assert (it == ex).mean() >= 0.99
    assert (stats["ext_steps"] > 256) == (name != "T110") and stats["to_plain"] >= 255
    # the fixture is what exact_iter_x gives: a handful of samples live
    for k in (0, 97, 255) if name != "E" else (0,):
        assert X.exact_iter_x(v, int(g["xs"][k]), int(g["ys"][k]), W, H) == ex[k], k
