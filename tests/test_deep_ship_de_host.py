"""Distance estimates for deep Burning Ship views (fr_render_deep_ship_de, fr_render_deepx_ship_de): the parts that need no GPU --
the ABI, validation, the Python wrapper, the restatement (tests/deep_ship_de_ref.py) against the restatements it extends, against
the Jacobian iterated directly in Python integers, against central differences of the exact orbit and, with Mandelbrot's L,
against deep_de_ref's complex derivative; and the registers of the four kernels.

Measured, restatement against the exact Jacobian at F + 64 bits, worst relative error of de over the sampled escaped pixels with
de >= 1e-3 pixel spacings (every 53rd pixel of the 48 x 36 frame, 33 pixels), plain / with the table:
  A       3.64e-12 / 5.63e-12   (25 escaped, 19 qualify)      B       5.25e-12 / 1.34e-12   (22 escaped, 15 qualify)
  S310    2.11e-11 / 1.71e-11   (20 escaped, 11 qualify)      S400    1.15e-11 / 4.08e-11   (23 escaped, 16 qualify)
  TIP400  1.35e-15 / 1.35e-15   (32 escaped, 32 qualify)      TIPY300 3.65e-15 / 2.09e-15   (33 escaped, 33 qualify)
  NUC546  every pixel of the frame is interior (the exact iteration agrees on all 33): de = 0, deriv = 0, nothing to bound.
On A and B the fp64 loop and the extended loop give the same bits, so the same figures.  The bounds below are four times the larger
figure of each view.  With L's signs taken from b's mantissas the extended step is wrong by 0.499 on TIP400, where Y = 0 exactly:
aligned to X's exponent, y = dz.y is 0 and its sign is gone in the one step where it is negative."""
import ctypes as C
import functools
import inspect
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import deep_de_ref as DE
import deep_isa
import deep_ref as R
import deep_ship_bla_ref as SB
import deep_ship_de_ref as SD
import deep_ship_ref as S
import deepx_ship_bla_ref as XSB
import deepx_ship_ref as XS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 48, 36
VIEWS = SD.views()


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _xview(v):
    return v if isinstance(v["zoom"], str) else XS.as_x_view(v)


@functools.lru_cache(maxsize=None)
def _orbit_x(name):
    return XS.orbit_of(_xview(VIEWS[name]))


@functools.lru_cache(maxsize=None)
def _restated_x(name, bla, w=W, h=H):
    """computed once, shared, never changed"""
    return SD.restate_x_de(_xview(VIEWS[name]), w, h, bla=bla, orbit=_orbit_x(name))


@functools.lru_cache(maxsize=None)
def _restated(name, bla, w=W, h=H):
    return SD.restate_de(VIEWS[name], w, h, bla=bla)


# ---- ABI -----------------------------------------------------------------------------------------------------------
NEW = ("fr_deep_ship_de_validate", "fr_deepx_ship_de_validate", "fr_render_deep_ship_de", "fr_render_deep_ship_de_async",
       "fr_render_deepx_ship_de", "fr_render_deepx_ship_de_async")


def test_abi_symbols_and_the_struct_they_share(fr, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "fractalrenderer_amd.h")).read()
    assert re.search(r"#define FR_HAS_DEEP_SHIP_DE 1", hdr) and re.search(r"#define FR_HAS_DEEPX_SHIP_DE 1", hdr)
    assert "Out of scope: the Burning Ship" not in hdr
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in fr._capi.SIGNATURES and hasattr(fr.lib(), name), name
    Sg, P, K = fr._capi.SIGNATURES, C.POINTER, fr._capi
    assert Sg["fr_deep_ship_de_validate"] == (C.c_int, [P(K.fr_params), P(K.fr_deep_view), P(K.fr_deep_de), C.c_uint32, C.c_uint32])
    assert Sg["fr_deepx_ship_de_validate"] == (C.c_int, [P(K.fr_params), P(K.fr_deepx_view), P(K.fr_deep_de), C.c_uint32, C.c_uint32])
    assert Sg["fr_render_deep_ship_de"][1] == Sg["fr_render_deep_de"][1]
    assert Sg["fr_render_deepx_ship_de"][1] == Sg["fr_render_deepx_de"][1]
    assert Sg["fr_render_deep_ship_de_async"][1] == Sg["fr_render_deep_ship_de"][1] + [C.c_void_p]
    assert Sg["fr_render_deepx_ship_de_async"][1] == Sg["fr_render_deepx_ship_de"][1] + [C.c_void_p]
    assert C.sizeof(K.fr_deep_de) == 24                           # reused unchanged
    gcc = shutil.which("gcc")
    if gcc:                                                       # the header compiles as C and declares the six
        src = tmp_path / "decl.c"
        src.write_text("#include \"fractalrenderer_amd.h\"\n"
                       "#if !defined(FR_HAS_DEEP_SHIP_DE) || FR_HAS_DEEP_SHIP_DE != 1 || FR_HAS_DEEPX_SHIP_DE != 1\n#error FR_HAS\n#endif\n"
                       "_Static_assert(sizeof(fr_deep_de) == 24, \"fr_deep_de\");\n"
                       "int (*a)(const fr_params*, const fr_deep_view*, const fr_deep_de*, uint32_t, uint32_t) = fr_deep_ship_de_validate;\n"
                       "int (*b)(const fr_params*, const fr_deepx_view*, const fr_deep_de*, uint32_t, uint32_t) = fr_deepx_ship_de_validate;\n"
                       "int (*c)(fr_ctx*, const fr_params*, const fr_deep_view*, const fr_deep_de*, uint32_t, uint32_t, const fr_shard*,\n"
                       "         const fr_output*) = fr_render_deep_ship_de;\n"
                       "int (*d)(fr_ctx*, const fr_params*, const fr_deep_view*, const fr_deep_de*, uint32_t, uint32_t, const fr_shard*,\n"
                       "         const fr_output*, void*) = fr_render_deep_ship_de_async;\n"
                       "int (*e)(fr_ctx*, const fr_params*, const fr_deepx_view*, const fr_deep_de*, uint32_t, uint32_t, const fr_shard*,\n"
                       "         const fr_output*) = fr_render_deepx_ship_de;\n"
                       "int (*f)(fr_ctx*, const fr_params*, const fr_deepx_view*, const fr_deep_de*, uint32_t, uint32_t, const fr_shard*,\n"
                       "         const fr_output*, void*) = fr_render_deepx_ship_de_async;\n")
        subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "decl.o")], check=True)


# ---- validation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [False, True], ids=["fp64", "extended"])
def test_validation_matrix(fr, ext):
    """every rule of the plain ship validator carries over with its status; then the distance block's own"""
    F = fr._capi
    L = fr.lib()
    plane = np.zeros(4, np.float64)
    de_validate = L.fr_deepx_ship_de_validate if ext else L.fr_deep_ship_de_validate
    validate = L.fr_deepx_ship_validate if ext else L.fr_deep_ship_validate
    mine, other = (F.FR_FLAG_DEEPX_SHIP_BLA, F.FR_FLAG_DEEP_SHIP_BLA) if ext else (F.FR_FLAG_DEEP_SHIP_BLA, F.FR_FLAG_DEEPX_SHIP_BLA)

    def mkview(cx=b"-1.75", cy=b"-0.03", zoom=b"1e-400", frac_bits=0, reserved=0):
        return F.fr_deepx_view(cx, cy, zoom, frac_bits, reserved) if ext else F.fr_deep_view(cx, cy, frac_bits, reserved)

    def params(**kw):
        p = fr.FractalState(zoom=1e-30).to_params(fr.FractalType.BurningShip, fr.Precision.F64)
        for k, val in kw.items():
            setattr(p, k, val)
        return p

    def check(Wd=64, Hd=48, view=None, de=None, **kw):
        p = params(**kw)
        view = view if view is not None else mkview()
        e = de if de is not None else F.fr_deep_de(plane.ctypes.data, None, 0, 1.8)
        return de_validate(C.byref(p), C.byref(view), C.byref(e), Wd, Hd), validate(C.byref(p), C.byref(view), Wd, Hd)

    OK, INV, UNS = F.FR_OK, F.FR_ERR_INVALID_ARG, F.FR_ERR_UNSUPPORTED
    assert check() == (OK, OK)
    assert check(flags=mine) == (OK, OK)
    assert check(flags=mine | F.FR_FLAG_POST_CHAIN) == (OK, OK)
    # the foreign BLA flags, as in the plain ship entry points
    foreign = [F.FR_FLAG_DEEP_BLA, F.FR_FLAG_DEEPX_BLA, F.FR_FLAG_DEEP_JULIA_BLA, F.FR_FLAG_DEEPX_JULIA_BLA]
    if ext:
        foreign.append(other)
    else:                                                         # fr_render_deep_ship does not read the extended ship's flag
        assert check(flags=other) == (OK, OK) and check(flags=mine | other) == (OK, OK)
    for f in foreign:
        assert check(flags=f) == (UNS, UNS), hex(f)
        assert check(flags=mine | f) == (UNS, UNS), hex(f)
    for kw in [dict(fractal_type=t) for t in (0, 1, 3, 4, 5, 99)] + [dict(precision=0), dict(orbit_trap_enabled=1),
                                                                       dict(interior_style=3), dict(stripe_enabled=1, interior_style=2)]:
        got = check(**kw)
        assert got == (UNS, UNS), (kw, got)
    invalid = [dict(Wd=0), dict(Hd=0), dict(Wd=65536, Hd=32768), dict(max_iterations=0), dict(max_iterations=(1 << 24) + 1),
               dict(antialiasing_samples=17), dict(antialiasing_samples=-1), dict(bailout=0.0), dict(bailout=float("nan")),
               dict(bailout=65537.0), dict(view=mkview(cx=b"1e")), dict(view=mkview(cy=b"")), dict(view=mkview(cx=None)),
               dict(view=mkview(reserved=3)), dict(view=mkview(frac_bits=100))]
    if ext:
        invalid += [dict(view=mkview(zoom=z)) for z in (b"9.999999999e-1001", b"1000.0000001", b"0", b"-1e-400", b"1e", None)]
    else:
        invalid += [dict(zoom=z) for z in (0.0, -1.0, 9e-291, 1001.0, float("nan"))]
    for kw in invalid:
        got = check(**kw)
        assert got == (INV, INV), (kw, got)
    # every bad fr_deep_de
    p, good = params(), mkview()
    blk = lambda *a: C.byref(F.fr_deep_de(*a))
    assert de_validate(C.byref(p), C.byref(good), None, 64, 48) == INV
    assert de_validate(None, C.byref(good), blk(None, None, 0, 1.8), 64, 48) == INV
    assert de_validate(C.byref(p), None, blk(None, None, 0, 1.8), 64, 48) == INV
    for shade in (2, -1, 256):
        assert check(de=F.fr_deep_de(None, None, shade, 1.8))[0] == INV, shade
    for edge in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert check(de=F.fr_deep_de(None, None, 1, edge))[0] == INV, edge
        assert check(de=F.fr_deep_de(None, None, 0, edge))[0] == OK, edge              # not read without the shading
    assert check(de=F.fr_deep_de(None, None, 1, 1e-30))[0] == OK
    assert check(flags=F.FR_FLAG_DEEP_BLA, de=F.fr_deep_de(None, None, 2, 1.8))[0] == UNS            # the view's rules come first
    e = F.fr_deep_de(1, 2, 7, 9.0)                                 # fr_deep_de_default composes with the new validators
    assert L.fr_deep_de_default(C.byref(e)) == 0
    assert de_validate(C.byref(p), C.byref(good), C.byref(e), 64, 48) == OK
    # the render entry points: a NULL context is an invalid argument
    o = F.fr_output(None, None, None, F.FR_MEM_HOST, 0)
    e = F.fr_deep_de(plane.ctypes.data, None, 0, 1.8)
    sync, asyn = (L.fr_render_deepx_ship_de, L.fr_render_deepx_ship_de_async) if ext else (L.fr_render_deep_ship_de, L.fr_render_deep_ship_de_async)
    assert sync(None, C.byref(p), C.byref(good), C.byref(e), 64, 48, None, C.byref(o)) == INV
    assert asyn(None, C.byref(p), C.byref(good), C.byref(e), 64, 48, None, C.byref(o), None) == INV


# ---- the Python wrapper ----------------------------------------------------------------------------------------------
def test_python_wrapper_signature_dispatch_and_host_plane_sizes(fr):
    sig = inspect.signature(fr.Renderer.render_deep_ship_de)
    names = list(sig.parameters)
    assert names == ["self", "state", "width", "height", "view", "post_chain", "rgba", "nu", "iter", "de", "deriv", "shade",
                     "edge_px", "shard", "stream", "sync", "bla"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["view"], d["post_chain"], d["shade"], d["edge_px"], d["sync"], d["bla"]) == (None, False, False, fr.DEEP_DE_EDGE_PX, True, False)
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names[5:])

    class Ctx:                                                    # a renderer without a context: the calls it would make
        calls = []

        class _lib:
            pass
        _ctx = None
        _output = fr.Renderer._output
        _ptr = staticmethod(fr.Renderer._ptr)

    def entry(name, is_async):
        def f(ctx, p, v, e, w, h, sh, out, *stream):
            Ctx.calls.append((name, p._obj.flags, p._obj.fractal_type, p._obj.precision, e._obj.shade, e._obj.edge_px, e._obj.de,
                              e._obj.deriv, getattr(v._obj, "zoom", None), stream[0].value if is_async else None, out._obj.memory))
            return 0
        return staticmethod(f)

    for n in NEW[2:]:
        setattr(Ctx._lib, n, entry(n, n.endswith("_async")))
    st = fr.FractalState(zoom=1e-30)
    de = np.zeros((4, 6), np.float64)
    deriv = np.zeros((4, 6, 4), np.float64)
    call = fr.Renderer.render_deep_ship_de
    ctx = Ctx()
    F = fr._capi
    call(ctx, st, 6, 4, de=de)
    call(ctx, st, 6, 4, fr.DeepView("0.1", "0.2"), de=de, deriv=deriv, shade=True, edge_px=0.25, bla=True, post_chain=True)
    call(ctx, st, 6, 4, fr.DeepView("0.1", "0.2", zoom="1e-400"), de=de, deriv=deriv, bla=True)
    call(ctx, st, 6, 4, fr.DeepView("0.1", "0.2", zoom="1e-400"), de=de, sync=False, stream=77)
    call(ctx, st, 6, 4, fr.DeepView("0.1", "0.2"), de=de, sync=False, stream=78, bla=True)
    B2 = int(fr.FractalType.BurningShip)
    assert Ctx.calls[0] == ("fr_render_deep_ship_de", 0, B2, F.FR_PRECISION_F64, 0, np.float32(1.8), de.ctypes.data, None, None, None,
                            F.FR_MEM_HOST)
    assert Ctx.calls[1][:10] == ("fr_render_deep_ship_de", F.FR_FLAG_DEEP_SHIP_BLA | F.FR_FLAG_POST_CHAIN, B2, F.FR_PRECISION_F64, 1, 0.25,
                                 de.ctypes.data, deriv.ctypes.data, None, None)
    assert Ctx.calls[2][:2] == ("fr_render_deepx_ship_de", F.FR_FLAG_DEEPX_SHIP_BLA) and Ctx.calls[2][8] == b"1e-400"
    assert Ctx.calls[2][7] == deriv.ctypes.data
    assert Ctx.calls[3][:2] == ("fr_render_deepx_ship_de_async", 0) and Ctx.calls[3][9] == 77
    assert Ctx.calls[4][:2] == ("fr_render_deep_ship_de_async", F.FR_FLAG_DEEP_SHIP_BLA) and Ctx.calls[4][9] == 78
    # host planes: deriv is rows * W * 4 doubles, nothing else is taken
    for bad in (np.zeros((4, 6, 2), np.float64), np.zeros((4, 6), np.float64), np.zeros((4, 6, 4), np.float32),
                np.zeros((3, 6, 4), np.float64)):
        with pytest.raises(ValueError):
            call(ctx, st, 6, 4, de=de, deriv=bad)
    with pytest.raises(ValueError):
        call(ctx, st, 6, 4, de=np.zeros((4, 6), np.float32))
    with pytest.raises(ValueError):
        call(ctx, st, 6, 4, de=de, stream=5)
    assert len(Ctx.calls) == 5


# ---- the restatement against the restatements it extends -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "TIPY300"])
def test_the_jacobian_feeds_nothing_back(name):
    """iter, r2 and the three counts of the loops with J are those of the loops without it, in both arithmetics"""
    v = VIEWS[name]
    w, h = 32, 24
    orb = _orbit_x(name)
    for bla in (False, True):
        (smp,), cnt = SD.restate_x_de(_xview(v), w, h, bla=bla, orbit=orb)
        if bla:
            ref, rc = XSB.restate_ship_x_bla(_xview(v), w, h, orbit=orb)
            assert rc == cnt
        else:
            ref = XS.restate_ship_x(_xview(v), w, h, orbit=orb)
        assert np.array_equal(ref[0][0], smp[0]) and np.array_equal(_u64(ref[0][1]), _u64(smp[1])), (name, bla)
        if isinstance(v["zoom"], str):
            continue
        (smp,), cnt = SD.restate_de(v, w, h, bla=bla)
        if bla:
            ref, rc = SB.restate_bla(v, w, h)
            assert rc == cnt
        else:
            ref = S.restate(v, w, h)[0]
        assert np.array_equal(ref[0][0], smp[0]) and np.array_equal(_u64(ref[0][1]), _u64(smp[1])), (name, bla)


@pytest.mark.parametrize("bla", [False, True], ids=["plain", "bla"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_the_two_restatements_are_bit_identical_on_a_view_both_accept(name, bla):
    v = VIEWS[name]
    it, r2, J, z = _restated(name, bla)[0][0]
    xit, xr2, xJ, xJe, xz = _restated_x(name, bla)[0][0]
    assert np.array_equal(it, xit) and (it < v["max_iter"]).any()
    assert np.array_equal(_u64(SD.de_of(it, r2, J, z, v["max_iter"])), _u64(SD.de_x_of(xit, xr2, xJ, xJe, xz, v["max_iter"])))
    assert np.array_equal(_u64(SD.deriv_of(it, J, v["max_iter"])), _u64(SD.deriv_x_of(xit, xJ, xJe, v["max_iter"])))


# ---- against the exact Jacobian ------------------------------------------------------------------------------------------------
DE_MIN = 1e-3
BOUND = {"A": 2.3e-11, "B": 2.1e-11, "S310": 8.5e-11, "S400": 1.7e-10, "TIP400": 5.4e-15, "TIPY300": 1.5e-14, "NUC546": 0.0}
ESCAPED = {"A": 25, "B": 22, "S310": 20, "S400": 23, "TIP400": 32, "TIPY300": 33, "NUC546": 0}


def sampled():
    """every 53rd pixel of the 48 x 36 frame: (ys, xs), 33 pixels"""
    k = np.arange(0, W * H, 53)
    return k // W, k % W


@functools.lru_cache(maxsize=None)
def _exact(name):
    """(iter, de) of the sampled pixels: computed once, shared, never changed"""
    ys, xs = sampled()
    ex = [SD.exact_de(VIEWS[name], int(x), int(y), W, H) for x, y in zip(xs, ys)]
    return np.array([e[0] for e in ex]), np.array([e[1] for e in ex])


@pytest.mark.parametrize("name", list(BOUND))
def test_restatement_against_the_exact_jacobian(name):
    v = VIEWS[name]
    ys, xs = sampled()
    assert len(ys) == 33
    eit, ede = _exact(name)
    esc = eit < v["max_iter"]
    q = esc & (ede >= DE_MIN)
    print(name, "escaped", int(esc.sum()), "qualify", int(q.sum()), "smallest exact de", float(ede[esc].min()) if esc.any() else None)
    assert int(esc.sum()) == ESCAPED[name]
    assert 2 * int(q.sum()) >= int(esc.sum())                     # at least half of the sampled escaped pixels qualify
    cases = [(True, b) for b in (False, True)] + ([] if isinstance(v["zoom"], str) else [(False, b) for b in (False, True)])
    for ext, bla in cases:
        if ext:
            it, r2, J, Je, z = _restated_x(name, bla)[0][0]
            de = SD.de_x_of(it, r2, J, Je, z, v["max_iter"])
            deriv = SD.deriv_x_of(it, J, Je, v["max_iter"])
        else:
            it, r2, J, z = _restated(name, bla)[0][0]
            de = SD.de_of(it, r2, J, z, v["max_iter"])
            deriv = SD.deriv_of(it, J, v["max_iter"])
        assert np.array_equal(it[ys, xs], eit), (name, ext, bla)
        assert np.all(np.isfinite(de)) and np.all(de[it == v["max_iter"]] == 0.0) and not deriv[it == v["max_iter"]].any()
        if not q.any():                                           # NUC546: all interior, the planes are zero
            assert not esc.any() and not de.any() and not deriv.any()
            continue
        rel = np.abs(de[ys, xs][q] - ede[q]) / ede[q]
        print(name, "extended" if ext else "fp64", "bla" if bla else "plain", "worst relative error", float(rel.max()), "bound", BOUND[name])
        assert float(rel.max()) <= BOUND[name], (name, ext, bla, float(rel.max()))


def test_the_signs_of_the_extended_step_cannot_come_from_the_aligned_sum():
    """TIP400: Y = 0 exactly, so y = dz.y, 2^-1330 below x.  A step that reads sgn y off b's mantissas misses the one update in
    which y is negative; the estimate is then wrong by half on the pixels below the axis"""
    v = VIEWS["TIP400"]
    ys, xs = sampled()
    eit, ede = _exact("TIP400")
    (smp,), _ = SD.restate_x_de(v, W, H, orbit=_orbit_x("TIP400"), signs_from_b=True)
    de = SD.de_x_of(*smp, v["max_iter"])
    esc = eit < v["max_iter"]
    rel = np.abs(de[ys, xs][esc] - ede[esc]) / ede[esc]
    assert rel.max() > 0.4


# ---- the convention, by finite differences ---------------------------------------------------------------------------------
def test_the_jacobian_is_the_derivative_of_the_exact_orbit():
    """central differences of the exact orbit in Fractions, h = 1e-30, at c = (-1.753, -0.031), n = 12, reproduce J / s; J is
    visibly not conformal there.  Independent of the restatement and of exact_de."""
    cx, cy, n = Fraction("-1.753"), Fraction("-0.031"), 12
    h = Fraction(1, 10 ** 30)
    xp, yp = SD.exact_orbit_fraction(cx + h, cy, n)
    xm, ym = SD.exact_orbit_fraction(cx - h, cy, n)
    xq, yq = SD.exact_orbit_fraction(cx, cy + h, n)
    xn, yn = SD.exact_orbit_fraction(cx, cy - h, n)
    fd = [(xp - xm) / (2 * h), (xq - xn) / (2 * h), (yp - ym) / (2 * h), (yq - yn) / (2 * h)]
    d = SD.jacobian_fraction(cx, cy, n)
    scale = max(abs(v) for v in d)
    err = max(abs(a - b) for a, b in zip(fd, d)) / scale
    print("finite differences against the recurrence:", float(err))
    assert err < Fraction(1, 10 ** 50)                            # the orbit is a polynomial on its piece: the error is O(h^2)
    assert abs(d[0] - d[3]) / scale > Fraction(1, 100) or abs(d[1] + d[2]) / scale > Fraction(1, 100)


# ---- the conformal case ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_with_mandelbrots_l_the_matrix_is_deep_de_refs_derivative(name):
    v = R.VIEWS[name]
    w, h = 32, 24
    orbit = R.reference_orbit(v["cx"], v["cy"], v["zoom"], v["max_iter"])
    dcx, dcy = R.sample_dc(w, h, v["zoom"], 1, 0)
    sp = DE.spacing(v["zoom"], h)
    it, r2, Dx, Dy, _ = DE.perturb_de(orbit, dcx, dcy, v["max_iter"], [], sp)
    jit, jr2, J, z, _ = SD.perturb_de(orbit, dcx, dcy, v["max_iter"], [], sp, lin=SD.mandel_l, fold=False)
    esc = it < v["max_iter"]
    assert esc.any() and np.array_equal(it, jit) and np.array_equal(_u64(r2), _u64(jr2))
    assert np.array_equal(_u64(J[..., 0][esc]), _u64(Dx[esc])) and np.array_equal(_u64(J[..., 3][esc]), _u64(Dx[esc]))
    assert np.array_equal(_u64(J[..., 2][esc]), _u64(Dy[esc])) and np.array_equal(_u64(J[..., 1][esc]), _u64(-Dy[esc]))
    a, b = SD.de_of(jit, jr2, J, z, v["max_iter"])[esc], DE.de_of(it, r2, Dx, Dy, v["max_iter"])[esc]
    rel = np.abs(a - b) / b
    print(name, "conformal de against deep_de_ref, worst relative difference", float(rel.max()))
    assert float(rel.max()) <= 2.0 ** -50


# ---- kernels -------------------------------------------------------------------------------------------------------
# The four kernels are deep_ship_de_kernel<DeepBlock<ShipFormula, X, true, BLA>>, keyed here by their own symbols.  A 512-VGPR
# file in granules of 8 gives 5 waves up to 96 VGPRs, 4 up to 128 and 3 up to 168.  Measured: (X, BLA) = (0, 0) 109 VGPRs and
# 4 waves per SIMD, (0, 1) 153 and 3, (1, 0) 125 and 4, (1, 1) 160 and 3; the kernels they extend have 89 / 5, 120 / 4,
# 101 / 4 and 130 / 3.  No scratch and no VGPR spill in any of them.
VGPRS = {(False, False): (109, 4), (False, True): (153, 3), (True, False): (125, 4), (True, True): (160, 3)}


def _ship_de_key(symbol):
    m = re.match(r"^_ZN2fr\d+deep_ship_de_kernelINS_\d+DeepBlockINS_\d+ShipFormulaELb([01])ELb1ELb([01])EEEEEvT_$", symbol)
    return ("ShipDe",) + tuple(b == "1" for b in m.group(1, 2)) if m else None


@functools.lru_cache(maxsize=None)
def _ship_de_kernels():
    """deep_isa's compile and parse with the new kernels' key in place of its own: their usage and assembly"""
    own = deep_isa.key_of
    deep_isa.key_of = _ship_de_key
    try:
        return deep_isa.kernels.__wrapped__()
    finally:
        deep_isa.key_of = own


def test_ship_de_kernels_use_no_scratch_and_stay_within_their_registers():
    built = _ship_de_kernels()
    if built is None:
        pytest.skip("hipcc not available")
    assert set(built) == {("ShipDe", x, b) for x in (False, True) for b in (False, True)}
    for (_, x, bla), k in sorted(built.items()):
        u = k.usage
        vg, occ = VGPRS[(x, bla)]
        print("deep_ship_de_kernel X", x, "BLA", bla, u)
        assert u["ScratchSize [bytes/lane]"] == 0 and u.get("VGPRs Spill", 0) == 0, (x, bla, u)
        assert u["VGPRs"] <= vg and u["Occupancy [waves/SIMD]"] >= occ, (x, bla, u)
