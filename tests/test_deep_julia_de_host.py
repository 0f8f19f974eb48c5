"""Distance estimates for deep Julia views (fr_render_deep_julia_de, fr_render_deepx_julia_de): the parts that need no GPU -- the
ABI, validation, the Python wrapper, the restatement (tests/deep_julia_de_ref.py) against the restatements it extends and
against the derivative iterated directly in Python integers, the flush of the extended derivative, and the register budget of
the four kernels."""
import ctypes as C
import functools
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import deep_isa
import deep_julia_bla_ref as JB
import deep_julia_de_ref as JD
import deep_julia_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 48, 36


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- ABI -----------------------------------------------------------------------------------------------------------
NEW = ("fr_deep_julia_de_validate", "fr_deepx_julia_de_validate", "fr_render_deep_julia_de", "fr_render_deep_julia_de_async",
       "fr_render_deepx_julia_de", "fr_render_deepx_julia_de_async")


def test_abi_symbols_and_the_struct_they_share(fr, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "fractalrenderer_amd.h")).read()
    assert re.search(r"#define FR_HAS_DEEP_JULIA_DE 1", hdr) and re.search(r"#define FR_HAS_DEEPX_JULIA_DE 1", hdr)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in fr._capi.SIGNATURES and hasattr(fr.lib(), name), name
    S, P, K = fr._capi.SIGNATURES, C.POINTER, fr._capi
    assert S["fr_deep_julia_de_validate"] == (C.c_int, [P(K.fr_params), P(K.fr_deep_view), P(K.fr_deep_de), C.c_uint32, C.c_uint32])
    assert S["fr_deepx_julia_de_validate"] == (C.c_int, [P(K.fr_params), P(K.fr_deepx_view), P(K.fr_deep_de), C.c_uint32, C.c_uint32])
    assert S["fr_render_deep_julia_de"][1] == S["fr_render_deep_de"][1]
    assert S["fr_render_deepx_julia_de"][1] == S["fr_render_deepx_de"][1]
    assert S["fr_render_deep_julia_de_async"][1] == S["fr_render_deep_julia_de"][1] + [C.c_void_p]
    assert S["fr_render_deepx_julia_de_async"][1] == S["fr_render_deepx_julia_de"][1] + [C.c_void_p]
    assert C.sizeof(K.fr_deep_de) == 24
    gcc = shutil.which("gcc")
    if gcc:                                                       # the header compiles as C and declares the six
        src = tmp_path / "decl.c"
        src.write_text("#include \"fractalrenderer_amd.h\"\n"
                       "#if !defined(FR_HAS_DEEP_JULIA_DE) || FR_HAS_DEEP_JULIA_DE != 1 || FR_HAS_DEEPX_JULIA_DE != 1\n#error FR_HAS\n#endif\n"
                       "int (*a)(const fr_params*, const fr_deep_view*, const fr_deep_de*, uint32_t, uint32_t) = fr_deep_julia_de_validate;\n"
                       "int (*b)(const fr_params*, const fr_deepx_view*, const fr_deep_de*, uint32_t, uint32_t) = fr_deepx_julia_de_validate;\n"
                       "int (*c)(fr_ctx*, const fr_params*, const fr_deep_view*, const fr_deep_de*, uint32_t, uint32_t, const fr_shard*,\n"
                       "         const fr_output*) = fr_render_deep_julia_de;\n"
                       "int (*d)(fr_ctx*, const fr_params*, const fr_deep_view*, const fr_deep_de*, uint32_t, uint32_t, const fr_shard*,\n"
                       "         const fr_output*, void*) = fr_render_deep_julia_de_async;\n"
                       "int (*e)(fr_ctx*, const fr_params*, const fr_deepx_view*, const fr_deep_de*, uint32_t, uint32_t, const fr_shard*,\n"
                       "         const fr_output*) = fr_render_deepx_julia_de;\n"
                       "int (*f)(fr_ctx*, const fr_params*, const fr_deepx_view*, const fr_deep_de*, uint32_t, uint32_t, const fr_shard*,\n"
                       "         const fr_output*, void*) = fr_render_deepx_julia_de_async;\n")
        subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "decl.o")], check=True)


# ---- validation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [False, True], ids=["fp64", "extended"])
def test_validation_matrix(fr, ext):
    """every rule of the plain Julia validator carries over with its status; then the distance block's own"""
    F = fr._capi
    L = fr.lib()
    plane = np.zeros(4, np.float64)
    de_validate = L.fr_deepx_julia_de_validate if ext else L.fr_deep_julia_de_validate
    validate = L.fr_deepx_julia_validate if ext else L.fr_deep_julia_validate
    mine, other = (F.FR_FLAG_DEEPX_JULIA_BLA, F.FR_FLAG_DEEP_JULIA_BLA) if ext else (F.FR_FLAG_DEEP_JULIA_BLA, F.FR_FLAG_DEEPX_JULIA_BLA)

    def mkview(cx=b"0.25", cy=b"0", zoom=b"1e-400", frac_bits=0, reserved=0):
        return F.fr_deepx_view(cx, cy, zoom, frac_bits, reserved) if ext else F.fr_deep_view(cx, cy, frac_bits, reserved)

    def params(**kw):
        p = fr.FractalState(zoom=1e-30, julia_c_real=-0.12, julia_c_imag=0.74).to_params(fr.FractalType.JuliaSet, fr.Precision.F64)
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
    assert check(flags=mine | F.FR_FLAG_POST_CHAIN) == (OK, OK)
    assert check(interior_style=2, orbit_trap_enabled=1, stripe_enabled=1) == (OK, OK)      # Julia has none of them: ignored
    unsupported = [dict(fractal_type=t) for t in (0, 2, 3, 4, 5, 99)] + [dict(precision=0), dict(flags=other), dict(flags=mine | other)]
    unsupported += [dict(flags=f) for f in (F.FR_FLAG_DEEP_BLA, F.FR_FLAG_DEEPX_BLA, F.FR_FLAG_DEEP_SHIP_BLA, F.FR_FLAG_DEEPX_SHIP_BLA)]
    unsupported += [dict(flags=mine | F.FR_FLAG_DEEP_BLA)]
    for kw in unsupported:
        assert check(**kw) == (UNS, UNS), kw
    invalid = [dict(Wd=0), dict(Hd=0), dict(Wd=65536, Hd=32768), dict(max_iterations=0), dict(max_iterations=(1 << 24) + 1),
               dict(antialiasing_samples=17), dict(antialiasing_samples=-1), dict(bailout=0.0), dict(bailout=float("nan")),
               dict(bailout=65537.0), dict(julia_c_real=float("inf")), dict(julia_c_imag=float("nan")), dict(julia_c_real=2.0 ** 32),
               dict(view=mkview(cx=b"1e")), dict(view=mkview(cy=b"")), dict(view=mkview(cx=None)), dict(view=mkview(reserved=3)),
               dict(view=mkview(frac_bits=100)), dict(view=mkview(cx=b"4.1")),          # the centre outside the bailout radius
               dict(view=mkview(cx=b"3", cy=b"3"))]
    if ext:
        invalid += [dict(view=mkview(zoom=z)) for z in (b"9.999999999e-1001", b"1000.0000001", b"0", b"-1e-400", b"1e", None)]
    else:
        invalid += [dict(zoom=z) for z in (0.0, -1.0, 9e-291, 1001.0, float("nan"))]
    for kw in invalid:
        assert check(**kw) == (INV, INV), kw
    assert check(view=mkview(cx=b"4"), bailout=4.0) == (OK, OK)   # on the radius: |centre|^2 == bailout^2 is inside
    # the block's rules
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
    assert check(flags=other, de=F.fr_deep_de(None, None, 2, 1.8))[0] == UNS            # the view's rules come first
    e = F.fr_deep_de(1, 2, 7, 9.0)                                 # fr_deep_de_default composes with the new validators
    assert L.fr_deep_de_default(C.byref(e)) == 0
    assert (e.de, e.deriv, e.shade) == (None, None, 0) and e.edge_px == np.float32(1.8)
    assert de_validate(C.byref(p), C.byref(good), C.byref(e), 64, 48) == OK
    # the render entry points: a NULL context is an invalid argument
    o = F.fr_output(None, None, None, F.FR_MEM_HOST, 0)
    e = F.fr_deep_de(plane.ctypes.data, None, 0, 1.8)
    sync, asyn = (L.fr_render_deepx_julia_de, L.fr_render_deepx_julia_de_async) if ext else (L.fr_render_deep_julia_de, L.fr_render_deep_julia_de_async)
    assert sync(None, C.byref(p), C.byref(good), C.byref(e), 64, 48, None, C.byref(o)) == INV
    assert asyn(None, C.byref(p), C.byref(good), C.byref(e), 64, 48, None, C.byref(o), None) == INV


# ---- the Python wrapper ----------------------------------------------------------------------------------------------
def test_python_wrapper_signature_and_dispatch(fr):
    sig = inspect.signature(fr.Renderer.render_deep_julia_de)
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
                              e._obj.deriv, getattr(v._obj, "zoom", None), stream[0].value if is_async else None))
            return 0
        return staticmethod(f)

    for n in NEW[2:]:
        setattr(Ctx._lib, n, entry(n, n.endswith("_async")))
    st = fr.FractalState(zoom=1e-30, julia_c_real=0.0, julia_c_imag=1.0)
    de = np.zeros((4, 6), np.float64)
    deriv = np.zeros((4, 6, 2), np.float64)
    call = fr.Renderer.render_deep_julia_de
    ctx = Ctx()
    F = fr._capi
    call(ctx, st, 6, 4, de=de)
    call(ctx, st, 6, 4, fr.DeepView("0.1", "0.2"), de=de, deriv=deriv, shade=True, edge_px=0.25, bla=True, post_chain=True)
    call(ctx, st, 6, 4, fr.DeepView("0.1", "0.2", zoom="1e-400"), de=de, bla=True)
    call(ctx, st, 6, 4, fr.DeepView("0.1", "0.2", zoom="1e-400"), de=de, sync=False, stream=77)
    call(ctx, st, 6, 4, fr.DeepView("0.1", "0.2"), de=de, sync=False, stream=78, bla=True)
    J1 = int(fr.FractalType.JuliaSet)
    assert Ctx.calls[0] == ("fr_render_deep_julia_de", 0, J1, F.FR_PRECISION_F64, 0, np.float32(1.8), de.ctypes.data, None, None, None)
    assert Ctx.calls[1] == ("fr_render_deep_julia_de", F.FR_FLAG_DEEP_JULIA_BLA | F.FR_FLAG_POST_CHAIN, J1, F.FR_PRECISION_F64, 1, 0.25,
                            de.ctypes.data, deriv.ctypes.data, None, None)
    assert Ctx.calls[2][:2] == ("fr_render_deepx_julia_de", F.FR_FLAG_DEEPX_JULIA_BLA) and Ctx.calls[2][8] == b"1e-400"
    assert Ctx.calls[3][:2] == ("fr_render_deepx_julia_de_async", 0) and Ctx.calls[3][9] == 77
    assert Ctx.calls[4][:2] == ("fr_render_deep_julia_de_async", F.FR_FLAG_DEEP_JULIA_BLA) and Ctx.calls[4][9] == 78
    with pytest.raises(ValueError):
        call(ctx, st, 6, 4, de=np.zeros((4, 6), np.float32))
    with pytest.raises(ValueError):
        call(ctx, st, 6, 4, de=de, deriv=np.zeros((4, 6), np.float64))
    with pytest.raises(ValueError):
        call(ctx, st, 6, 4, de=de, stream=5)
    assert len(Ctx.calls) == 5


# ---- the restatement against the restatements it extends -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["RABBIT30", "DUST30", "PRECRIT60"])
def test_the_derivative_feeds_nothing_back(name):
    """iter, r2 and the three counts of the loops with D are those of the loops without it, in both arithmetics"""
    v = JD.view(name)
    w, h = 32, 24
    for bla in (False, True):
        smp, cnt = JD.restated(name, w, h, 1, bla)
        xsmp, xcnt = JD.restated_x(name, w, h, 1, bla)
        if bla:
            base, bcnt = JB.restate_bla(v, w, h, orbits=JD.orbits(name))
            xbase, xbcnt = JB.restate_x_bla(v, w, h, orbits=JD.orbits_x(name))
            assert cnt == bcnt and xcnt == xbcnt
        else:
            base = J.restate(v, w, h, orbits=JD.orbits(name))
            xbase = J.restate_x(v, w, h, orbits=JD.orbits_x(name))
        assert np.array_equal(smp[0][0], base[0][0]) and np.array_equal(_u64(smp[0][1]), _u64(base[0][1]))
        assert np.array_equal(xsmp[0][0], xbase[0][0]) and np.array_equal(_u64(xsmp[0][1]), _u64(xbase[0][1]))


@pytest.mark.parametrize("name", ["RABBIT30", "DENDRITE100"])
def test_the_two_restatements_are_bit_identical_on_a_view_both_accept(name):
    """d0 is at least 2^-400 and no intermediate leaves a double's range: scaling by a power of two is exact"""
    v = JD.view(name)
    it, r2, Dx, Dy = JD.restated(name, W, H)[0][0]
    xit, xr2, xDx, xDy, xeD = JD.restated_x(name, W, H)[0][0]
    assert np.array_equal(it, xit)
    assert np.array_equal(_u64(JD.deriv_of(it, Dx, Dy, v["max_iter"])), _u64(JD.deriv_of_x(xit, xDx, xDy, xeD, v["max_iter"])))
    assert np.array_equal(_u64(JD.de_of(it, r2, Dx, Dy, v["max_iter"])), _u64(JD.de_of_x(xit, xr2, xDx, xDy, xeD, v["max_iter"])))


def test_an_escape_at_update_0_is_one_product():
    """D = 2 z_0 s: w.x s - w.y 0 and w.x 0 + w.y s, each exact or one rounding"""
    v = dict(JD.view("DENDRITE30"), cx="1.2", cy="0.25", zoom=0.05, zoom_s="0.05", F=128)      # inside bailout 1.25, P_1 outside
    w, h = 21, 13
    (it, r2, Dx, Dy), = JD.restate_de(v, w, h, bailout=1.25)[0]
    assert np.all(it == 0)
    d0x, d0y = JD.S.sample_dc(w, h, 0.05, 1, 0)
    s = JD.spacing(0.05, h)
    zx, zy = np.float64(1.2) + d0x, np.float64(0.25) + d0y
    assert np.array_equal(_u64(Dx), _u64((zx + zx) * s)) and np.array_equal(_u64(Dy), _u64((zy + zy) * s))


# ---- the restatement against the exact derivative ------------------------------------------------------------------------------
# Only escaped pixels whose exact de is at least DE_MIN pixel spacings are compared: below it the error of any fp64 iteration grows
# like 2^-53 / de (the orbit hugs the set for many updates after its delta has reached the size of z).  What keeps the filter from
# hiding a failure: QUALIFY, the number of the 33 sampled pixels (every 53rd of the 48 x 36 frame) that must qualify, and every
# sampled iter equal to the exact one.
# BOUND = 4 x the worst relative error measured on the qualifying pixels (plain and flagged, fp64 and extended loop alike),
# rounded up to one digit; the margin covers the libm log of another machine.  Measured, plain / flagged:
#   RABBIT30 5.79e-12 / 5.53e-12   DENDRITE30 8.83e-13 / 1.00e-12   DUST30 2.35e-10 / 2.99e-10 (at de = 1.2e-3)
#   DENDRITE100 1.15e-12 / 1.16e-12   DENDRITE400 1.11e-11 / 1.07e-11   DENDRITE1000 1.01e-9 / 3.75e-10
# and the same figures through the extended loop on the four views a double holds (the two loops are bit-identical there).
DE_MIN = 1e-3
QUALIFY = {"RABBIT30": 10, "DENDRITE30": 33, "DUST30": 31, "DENDRITE100": 33, "DENDRITE400": 32, "DENDRITE1000": 33}
BOUND = {"RABBIT30": 3e-11, "DENDRITE30": 5e-12, "DUST30": 2e-9, "DENDRITE100": 5e-12, "DENDRITE400": 5e-11, "DENDRITE1000": 5e-9}
EXACT_CASES = [(n, x) for n in ("RABBIT30", "DENDRITE30", "DUST30", "DENDRITE100") for x in (False, True)] + \
              [("DENDRITE400", True), ("DENDRITE1000", True)]


@functools.lru_cache(maxsize=None)
def _exact(name, ext):
    """(iter, de) of the sampled pixels: computed once (DENDRITE1000: 0.6 s a sample at 3520 bits), shared, never changed"""
    v = JD.view(name)
    ys, xs = JD.sampled(W, H)
    f = JD.exact_de_x if ext else JD.exact_de
    ex = [f(v, int(x), int(y), W, H) for x, y in zip(xs, ys)]
    return np.array([e[0] for e in ex]), np.array([e[1] for e in ex])


@pytest.mark.parametrize("name,ext", EXACT_CASES, ids=["%s-%s" % (n, "extended" if x else "fp64") for n, x in EXACT_CASES])
def test_restatement_against_the_exact_derivative(name, ext):
    v = JD.view(name)
    ys, xs = JD.sampled(W, H)
    assert len(ys) == 33
    eit, ede = _exact(name, ext)
    esc = eit < v["max_iter"]
    q = esc & (ede >= DE_MIN)
    print(name, "escaped", int(esc.sum()), "qualify", int(q.sum()), "smallest exact de", float(ede[esc].min()))
    assert int(q.sum()) >= QUALIFY[name] and (name != "RABBIT30" or int(esc.sum()) == 10)
    if not ext:                                                   # the two exact iterations start from the same point and spacing
        xit, xde = _exact(name, True)
        assert np.array_equal(eit, xit) and np.array_equal(ede, xde)
    for bla in (False, True):
        if ext:
            it, r2, Dx, Dy, eD = JD.restated_x(name, W, H, 1, bla)[0][0]
            de = JD.de_of_x(it, r2, Dx, Dy, eD, v["max_iter"])
        else:
            it, r2, Dx, Dy = JD.restated(name, W, H, 1, bla)[0][0]
            de = JD.de_of(it, r2, Dx, Dy, v["max_iter"])
        assert np.array_equal(it[ys, xs], eit), (name, bla)
        rel = np.abs(de[ys, xs][q] - ede[q]) / ede[q]
        print(name, "extended" if ext else "fp64", "bla" if bla else "plain", "worst relative error", float(rel.max()), "bound", BOUND[name])
        assert float(rel.max()) <= BOUND[name], (name, bla, float(rel.max()))


def test_the_frames_are_what_the_estimate_is_for():
    """63 % of the escaped pixels of DUST30 and 49 % of RABBIT30 lie less than one pixel spacing from the set"""
    for name, share in (("DUST30", 0.63), ("RABBIT30", 0.49)):
        v = JD.view(name)
        it, r2, Dx, Dy = JD.restated(name, W, H)[0][0]
        de = JD.de_of(it, r2, Dx, Dy, v["max_iter"])
        esc = it < v["max_iter"]
        assert abs(float((de[esc] < 1.0).mean()) - share) < 0.005, name


def test_precrit200_escapes_and_its_derivative_dips():
    """at least 90 % of the 32 x 24 pixels escape, and D's exponent drops by about 650 in one update and climbs back"""
    v = JD.view("PRECRIT200")
    stats = {}
    (smp,), _ = JD.restate_x_de(v, 32, 24, orbits=JD.orbits_x("PRECRIT200"), stats=stats)
    it, r2, Dx, Dy, eD = smp
    esc = it < v["max_iter"]
    assert esc.mean() >= 0.9
    es = JD.spacing_x(*JD.X.zoom_pair(v["zoom_s"]), 24)[1]
    assert stats["e_min"] < es - 600 and stats["d_flushes"] == 0
    assert np.all(eD[esc] > es + 600)                            # it climbed back, and well past where it started
    de = JD.de_of_x(it, r2, Dx, Dy, eD, v["max_iter"])
    assert np.all(np.isfinite(de[esc])) and np.all(de[esc] > 0.0)


# ---- the flush ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bla", [False, True], ids=["plain", "bla"])
@pytest.mark.parametrize("c", [(0.0, 0.0), (-1.0, 0.0)], ids=["c0", "c-1"])
def test_the_flush_of_the_extended_derivative(c, bla):
    """c = 0 and c = -1 at max_iterations 64: |2 z| squares itself towards nothing, D.e crosses -2^27 and D becomes the zero,
    while no exponent sum of a D update leaves (-2^29, 2^29) -- on the restatement's recorded extremes"""
    v = JD.basin_view(c)
    stats = {}
    (smp,), _ = JD.restate_x_de(v, 21, 13, bla=bla, stats=stats)
    it, r2, Dx, Dy, eD = smp
    print(stats)
    assert stats["d_flushes"] > 0 and stats["e_min"] < JD.X_FLUSH
    assert -(1 << 29) < stats["sum_min"] and stats["sum_max"] < (1 << 29)
    assert stats["e_max"] < 18 * (1 << 24)
    interior = it == v["max_iter"]
    assert interior.any()
    if c == (0.0, 0.0):
        assert interior.all()
    else:
        esc = ~interior
        assert esc.any()                                           # samples outside the basilica escape with a live D
        assert np.all(eD[esc] > JD.X_FLUSH) and np.all(np.isfinite(JD.de_of_x(it, r2, Dx, Dy, eD, v["max_iter"])[esc]))


def test_a_zero_derivative_gives_an_infinite_estimate():
    one = np.zeros(1, np.int32)
    assert JD.de_of(one, np.array([16.0]), np.array([0.0]), np.array([0.0]), 1)[0] == np.inf
    assert JD.de_of_x(one, np.array([16.0]), np.array([0.0]), np.array([0.0]), np.array([JD.X_ZERO]), 1)[0] == np.inf
    assert not JD.deriv_of_x(one, np.array([0.0]), np.array([0.0]), np.array([JD.X_ZERO]), 1).any()


# ---- kernels -------------------------------------------------------------------------------------------------------
# name -> (the kernel it extends, that kernel's VGPRs and waves per SIMD), under the blocks' names when these numbers were
# recorded (deep_isa.OLD_NAMES).  A 512-VGPR file in granules of 8 gives 5 waves up to
# 96 VGPRs, 4 up to 128 and 3 up to 168.  Measured: DeepJuliaDeArgs 95 VGPRs and 5 waves, DeepJuliaDeBlaArgs 127 and 4 (both keep
# their parent's occupancy), DeepJuliaXDeArgs 105 and 4, DeepJuliaXDeBlaArgs 143 and 3 (a wave less, as fr_render_deepx_de's pair).
# No scratch and no VGPR spill in any of them.
PARENT = {"DeepJuliaDeArgs": ("DeepJuliaArgs", 87, 5), "DeepJuliaDeBlaArgs": ("DeepJuliaBlaArgs", 115, 4),
          "DeepJuliaXDeArgs": ("DeepJuliaXArgs", 93, 5), "DeepJuliaXDeBlaArgs": ("DeepJuliaXBlaArgs", 126, 4)}


def test_julia_de_kernels_keep_their_register_budget(fr):
    built = deep_isa.by_old_name()
    if built is None:
        pytest.skip("hipcc not available")
    usage = {name: k.usage for name, k in built.items()}
    for name, (parent, parent_vgprs, parent_occ) in PARENT.items():
        u, pu = usage[name], usage[parent]
        print(name, u, "extends", parent, pu)
        assert (pu["VGPRs"], pu["Occupancy [waves/SIMD]"]) == (parent_vgprs, parent_occ), (parent, pu)
        assert u["ScratchSize [bytes/lane]"] == 0 and u.get("VGPRs Spill", 0) == 0, (name, u)
        assert u["Occupancy [waves/SIMD]"] >= parent_occ - 1, (name, u, pu)
