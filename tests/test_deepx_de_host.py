"""Distance estimates for extended views (fr_render_deepx_de): the parts that need no GPU -- the ABI, validation, the Python
wrapper, the restatement (tests/deepx_de_ref.py) against the restatements it extends, against fr_render_deep_de's on shallow
views and against the direct iteration of z^2 + c and its derivative in Python integers, and the register budget of the two
kernels."""
import ctypes as C
import functools
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import deep_de_ref as D
import deep_isa
import deep_ref as R
import deepx_bla_ref as XB
import deepx_de_ref as XD
import deepx_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS = X.views()
TIP400 = dict(cx="-2", cy="0", zoom="1e-400", max_iter=1400)
TIP1000 = dict(cx="-2", cy="0", zoom="1e-1000", max_iter=3400)
ALL = dict(VIEWS, tip400=TIP400, tip1000=TIP1000)


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _orbit(name):
    return X.orbit_of(ALL[name])


@functools.lru_cache(maxsize=None)
def _restated(name, w, h, bla=False):
    """computed once per case, shared, never changed"""
    return XD.restate_x_de(ALL[name], w, h, bla=bla, orbit=_orbit(name))


# ---- ABI -----------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_the_struct_it_shares(fr, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "fractalrenderer_amd.h")).read()
    assert re.search(r"#define FR_HAS_DEEPX_DE 1", hdr)
    for name in ("fr_deepx_de_validate", "fr_render_deepx_de", "fr_render_deepx_de_async"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in fr._capi.SIGNATURES and hasattr(fr.lib(), name), name
    S = fr._capi.SIGNATURES
    P = C.POINTER
    K = fr._capi
    assert S["fr_deepx_de_validate"] == (C.c_int, [P(K.fr_params), P(K.fr_deepx_view), P(K.fr_deep_de), C.c_uint32, C.c_uint32])
    assert S["fr_render_deepx_de"][1][1:4] == [P(K.fr_params), P(K.fr_deepx_view), P(K.fr_deep_de)]
    assert S["fr_render_deepx_de_async"][1] == S["fr_render_deepx_de"][1] + [C.c_void_p]
    assert C.sizeof(K.fr_deep_de) == 24 and C.sizeof(K.fr_deepx_view) == 32
    gcc = shutil.which("gcc")
    if gcc:                                                       # the header compiles as C and declares the three
        src = tmp_path / "decl.c"
        src.write_text("#include \"fractalrenderer_amd.h\"\n#if !defined(FR_HAS_DEEPX_DE) || FR_HAS_DEEPX_DE != 1\n#error FR_HAS_DEEPX_DE\n#endif\n"
                       "int (*a)(const fr_params*, const fr_deepx_view*, const fr_deep_de*, uint32_t, uint32_t) = fr_deepx_de_validate;\n"
                       "int (*b)(fr_ctx*, const fr_params*, const fr_deepx_view*, const fr_deep_de*, uint32_t, uint32_t, const fr_shard*,\n"
                       "         const fr_output*) = fr_render_deepx_de;\n"
                       "int (*c)(fr_ctx*, const fr_params*, const fr_deepx_view*, const fr_deep_de*, uint32_t, uint32_t, const fr_shard*,\n"
                       "         const fr_output*, void*) = fr_render_deepx_de_async;\n")
        subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "decl.o")], check=True)
    e = K.fr_deep_de(1, 2, 7, 9.0)                                 # fr_deep_de_default is unchanged
    assert fr.lib().fr_deep_de_default(C.byref(e)) == 0
    assert (e.de, e.deriv, e.shade) == (None, None, 0) and e.edge_px == np.float32(1.8)


# ---- validation ----------------------------------------------------------------------------------------------------
def _xview(fr, cx=b"-0.5", cy=b"0", zoom=b"1e-400", frac_bits=0, reserved=0):
    return fr._capi.fr_deepx_view(cx, cy, zoom, frac_bits, reserved)


def test_validation_matrix(fr):
    F = fr._capi
    L = fr.lib()
    plane = np.zeros(4, np.float64)

    def params(**kw):
        p = fr.FractalState(zoom=1.0).to_params(fr.FractalType.Mandelbrot, fr.Precision.F64)
        for k, val in kw.items():
            setattr(p, k, val)
        return p

    def check(W=64, H=48, view=None, de=None, **kw):
        p = params(**kw)
        view = view if view is not None else _xview(fr)
        e = de if de is not None else F.fr_deep_de(plane.ctypes.data, None, 0, 1.8)
        return L.fr_deepx_de_validate(C.byref(p), C.byref(view), C.byref(e), W, H), L.fr_deepx_validate(C.byref(p), C.byref(view), W, H)

    OK, INV, UNS = F.FR_OK, F.FR_ERR_INVALID_ARG, F.FR_ERR_UNSUPPORTED
    assert check() == (OK, OK)
    assert check(flags=F.FR_FLAG_DEEPX_BLA | F.FR_FLAG_POST_CHAIN) == (OK, OK)
    for zoom in (b"1e-1000", b"1e3", b"1e-30", b"3"):
        assert check(view=_xview(fr, zoom=zoom)) == (OK, OK), zoom
    assert check(zoom=1e-300, center_x=float("nan"), interior_style=1) == (OK, OK)          # p->zoom and the double centre are not read
    # every case fr_deepx_validate refuses is refused here, with its status
    unsupported = [dict(fractal_type=t) for t in (1, 2, 3, 4, 5, 99)] + [
        dict(precision=0), dict(orbit_trap_enabled=1), dict(stripe_enabled=1), dict(interior_style=2),
        dict(flags=F.FR_FLAG_DEEP_BLA), dict(flags=F.FR_FLAG_DEEP_JULIA_BLA), dict(flags=F.FR_FLAG_DEEPX_JULIA_BLA),
        dict(flags=F.FR_FLAG_DEEPX_BLA | F.FR_FLAG_DEEP_BLA), dict(flags=F.FR_FLAG_DEEPX_BLA | F.FR_FLAG_DEEPX_JULIA_BLA)]
    for kw in unsupported:
        assert check(**kw) == (UNS, UNS), kw
    invalid = [dict(W=0), dict(H=0), dict(W=65536, H=32768), dict(max_iterations=0), dict(max_iterations=(1 << 24) + 1),
               dict(antialiasing_samples=17), dict(antialiasing_samples=-1), dict(bailout=0.0), dict(bailout=float("nan")),
               dict(bailout=65537.0), dict(julia_c_real=float("inf")),
               dict(view=_xview(fr, zoom=b"9.999999999e-1001")), dict(view=_xview(fr, zoom=b"1000.0000001")),
               dict(view=_xview(fr, zoom=b"0")), dict(view=_xview(fr, zoom=b"-1e-400")), dict(view=_xview(fr, zoom=b"1e")),
               dict(view=_xview(fr, zoom=None)), dict(view=_xview(fr, cx=b"1e")), dict(view=_xview(fr, cy=b"")),
               dict(view=_xview(fr, cx=None)), dict(view=_xview(fr, reserved=3)), dict(view=_xview(fr, frac_bits=100)),
               dict(view=_xview(fr, frac_bits=4097)), dict(view=_xview(fr, cx=b"1" * 4097)), dict(view=_xview(fr, cx=b"4294967296"))]
    for kw in invalid:
        assert check(**kw) == (INV, INV), kw
    # the other BLA flags: fr_render_deepx does not read the ship's two, this entry point refuses all five
    for flag in (F.FR_FLAG_DEEP_BLA, F.FR_FLAG_DEEP_SHIP_BLA, F.FR_FLAG_DEEPX_SHIP_BLA, F.FR_FLAG_DEEP_JULIA_BLA,
                 F.FR_FLAG_DEEPX_JULIA_BLA):
        assert check(flags=flag)[0] == UNS, flag
        assert check(flags=flag | F.FR_FLAG_DEEPX_BLA)[0] == UNS, flag
    assert check(flags=F.FR_FLAG_DEEPX_SHIP_BLA, bailout=0.0)[0] == INV              # behind fr_render_deepx's own checks
    # the block's rules, fr_deep_de_validate's
    p, good = params(), _xview(fr)
    assert L.fr_deepx_de_validate(C.byref(p), C.byref(good), None, 64, 48) == INV
    assert L.fr_deepx_de_validate(None, C.byref(good), C.byref(F.fr_deep_de(None, None, 0, 1.8)), 64, 48) == INV
    assert L.fr_deepx_de_validate(C.byref(p), None, C.byref(F.fr_deep_de(None, None, 0, 1.8)), 64, 48) == INV
    for shade in (2, -1, 256):
        assert check(de=F.fr_deep_de(None, None, shade, 1.8))[0] == INV, shade
    for edge in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert check(de=F.fr_deep_de(None, None, 1, edge))[0] == INV, edge
        assert check(de=F.fr_deep_de(None, None, 0, edge))[0] == OK, edge              # not read without the shading
    assert check(de=F.fr_deep_de(None, None, 1, 1e-30))[0] == OK
    assert check(de=F.fr_deep_de(None, None, 1, 0.25))[0] == OK                       # the planes are the render's business
    # the render entry points: a NULL context, params, view or de is an invalid argument
    o = F.fr_output(None, None, None, F.FR_MEM_HOST, 0)
    e = F.fr_deep_de(plane.ctypes.data, None, 0, 1.8)
    assert L.fr_render_deepx_de(None, C.byref(p), C.byref(good), C.byref(e), 64, 48, None, C.byref(o)) == INV
    assert L.fr_render_deepx_de_async(None, C.byref(p), C.byref(good), C.byref(e), 64, 48, None, C.byref(o), None) == INV


# ---- the Python wrapper ----------------------------------------------------------------------------------------------
def test_python_wrapper_signature_flags_and_the_value_errors(fr):
    sig = inspect.signature(fr.Renderer.render_deepx_de)
    names = list(sig.parameters)
    assert names == ["self", "state", "width", "height", "view", "post_chain", "rgba", "nu", "iter", "de", "deriv", "shade",
                     "edge_px", "shard", "stream", "sync", "bla"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["view"] is inspect.Parameter.empty
    assert (d["post_chain"], d["shade"], d["edge_px"], d["sync"], d["bla"]) == (False, False, fr.DEEP_DE_EDGE_PX, True, False)
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names[5:])

    class Ctx:                                                    # a renderer without a context: the calls it would make
        calls = []

        class _lib:
            @staticmethod
            def fr_render_deepx_de(ctx, p, v, e, w, h, sh, out):
                Ctx.calls.append(("sync", p._obj.flags, p._obj.fractal_type, p._obj.precision, e._obj.shade, e._obj.edge_px,
                                  e._obj.de, e._obj.deriv, out._obj.memory, out._obj.rgba, v._obj.zoom))
                return 0

            @staticmethod
            def fr_render_deepx_de_async(ctx, p, v, e, w, h, sh, out, stream):
                Ctx.calls.append(("async", p._obj.flags, stream.value))
                return 0
        _ctx = None
        _output = fr.Renderer._output
        _ptr = staticmethod(fr.Renderer._ptr)

    st = fr.FractalState(zoom=1e-30)
    de = np.zeros((4, 6), np.float64)
    deriv = np.zeros((4, 6, 2), np.float64)
    call = fr.Renderer.render_deepx_de
    ctx = Ctx()
    view = fr.DeepView("0", "0", zoom="1e-400")
    call(ctx, st, 6, 4, view, de=de)
    call(ctx, st, 6, 4, view, de=de, deriv=deriv, shade=True, edge_px=0.25, bla=True, post_chain=True)
    call(ctx, st, 6, 4, view, de=de, sync=False, stream=77, bla=True)
    F = fr._capi
    assert Ctx.calls[0] == ("sync", 0, 0, F.FR_PRECISION_F64, 0, np.float32(1.8), de.ctypes.data, None, F.FR_MEM_HOST, None, b"1e-400")
    assert Ctx.calls[1][:6] == ("sync", F.FR_FLAG_DEEPX_BLA | F.FR_FLAG_POST_CHAIN, 0, F.FR_PRECISION_F64, 1, 0.25)
    assert Ctx.calls[1][6:8] == (de.ctypes.data, deriv.ctypes.data)
    assert Ctx.calls[2] == ("async", F.FR_FLAG_DEEPX_BLA, 77)
    with pytest.raises(ValueError, match="zoom string"):
        call(ctx, st, 6, 4, fr.DeepView("0", "0"), de=de)
    with pytest.raises(ValueError, match="zoom string"):
        call(ctx, st, 6, 4, None, de=de)
    with pytest.raises(ValueError):
        call(ctx, st, 6, 4, view, de=np.zeros((4, 6), np.float32))
    with pytest.raises(ValueError):
        call(ctx, st, 6, 4, view, de=de, deriv=np.zeros((4, 6), np.float64))
    with pytest.raises(ValueError):
        call(ctx, st, 6, 4, view, de=de, stream=5)
    assert len(Ctx.calls) == 3
    with pytest.raises(ValueError, match="render_deepx_de"):       # render_deep_de still refuses a zoom string, and says where to go
        fr.Renderer.render_deep_de(ctx, st, 6, 4, view, de=de)


# ---- the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["T130", "T300", "D"])
def test_planes_do_not_depend_on_the_derivative(name):
    """(iter, r2) of the restatement are deepx_ref.perturb_x's without a table and deepx_bla_ref.perturb_x_bla's with one, bit
    for bit, and so are the step counts"""
    v = ALL[name]
    w, h = 32, 24
    mant, exp2 = _orbit(name)
    zm, ze = X.zoom_pair(v["zoom"])
    (s,), _ = _restated(name, w, h)
    it, r2 = X.perturb_x(mant, exp2, X.sample_dc_x(w, h, zm, ze, 1, 0), v["max_iter"])
    assert np.array_equal(s[0].ravel(), it) and np.array_equal(_u64(s[1].ravel()), _u64(r2))
    (s,), counts = _restated(name, w, h, True)
    table = XB.bla_table_x(mant, exp2, XB.dcmax_x(w, h, zm, ze))
    it, r2, bcounts = XB.perturb_x_bla(mant, exp2, X.sample_dc_x(w, h, zm, ze, 1, 0), v["max_iter"], table)
    assert np.array_equal(s[0].ravel(), it) and np.array_equal(_u64(s[1].ravel()), _u64(r2)) and counts == bcounts
    assert counts[1] > 0


def test_first_update_and_interior():
    """D after the first update is (sm, 0, es) exactly, whatever the sample; interior samples have de 0 and deriv (0, 0)"""
    v = dict(VIEWS["D"], max_iter=1)
    w, h = 48, 36
    sm, es = XD.spacing_x(*X.zoom_pair(v["zoom"]), h)
    assert 0.5 <= sm < 1.0 and es < -1330
    (smp,), _ = XD.restate_x_de(v, w, h, bailout=1e-3)             # every sample escapes at once
    it, r2, Dx, Dy, eD = smp
    assert np.all(it == 0) and np.all(Dx == sm) and np.all(Dy == 0.0) and np.all(eD == es)
    (smp,), _ = XD.restate_x_de(v, w, h)                           # none does
    it, r2, Dx, Dy, eD = smp
    assert np.all(it == 1) and not XD.de_of_x(it, r2, Dx, Dy, eD, 1).any() and not XD.deriv_of_x(it, Dx, Dy, eD, 1).any()


@pytest.mark.parametrize("name", ["A", "B"])
def test_shallow_views_are_fr_render_deep_des_bit_for_bit(name):
    """VIEW_A (1e-30) and VIEW_B (1e-100) as extended views, without BLA: iter, r2, de and deriv of the restatement are
    deep_de_ref.restate_de's bit for bit -- scaling by a power of two is exact, so the extended D is the fp64 D with its
    exponent held apart"""
    v = dict(A=R.VIEW_A, B=R.VIEW_B)[name]
    zs = dict(A="1e-30", B="1e-100")[name]
    assert float(zs) == v["zoom"]
    w, h = 48, 36
    (xs,), _ = XD.restate_x_de(dict(v, zoom=zs), w, h)
    (ps,), _ = D.restate_de(v, w, h)
    it, r2, Dx, Dy, eD = xs
    pit, pr2, pDx, pDy = ps
    assert (pit < v["max_iter"]).sum() >= 100
    assert np.array_equal(it, pit) and np.array_equal(_u64(r2), _u64(pr2))
    assert np.array_equal(_u64(XD.de_of_x(it, r2, Dx, Dy, eD, v["max_iter"])), _u64(D.de_of(pit, pr2, pDx, pDy, v["max_iter"])))
    assert np.array_equal(_u64(XD.deriv_of_x(it, Dx, Dy, eD, v["max_iter"])), _u64(D.deriv_of(pit, pDx, pDy, v["max_iter"])))


EXACT_CASES = [("T110", 48, 36, 53), ("T130", 48, 36, 53), ("T300", 48, 36, 53), ("D", 48, 36, 53), ("E", 48, 36, 53),
               ("tip400", 21, 13, 9), ("tip1000", 21, 13, 9)]


@pytest.mark.parametrize("name,w,h,stride", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_restatement_agrees_with_the_exact_derivative(name, w, h, stride):
    """The restatement against exact_de_x (z^2 + c and d <- 2 z d + 1 in Python integers at F + 64 fraction bits) on every
    53rd pixel of the 48 x 36 views (33 samples) and every 9th of the 21 x 13 tip (31 samples).  Escape indices are equal on
    every sample tried (none is left out; at most 2 % may be), and |de - exact| / exact <= 1e-10, the bound of
    test_deep_de_host.py for the fp64 path.  Measured here, restatement against exact, worst per view: T110 1.8e-12,
    T130 4.5e-12, T300 8.1e-12, D 4.3e-12, E 2.5e-11, tip 1e-400 2.4e-15, tip 1e-1000 1.1e-15; no escape index differs.
    (A denser sampling finds worse pixels close to the set -- all 768 of D at 32 x 24: 3.3e-10, see BLA_BOUND below -- but this
    test's samples are these, and its bound stays the fp64 path's.)"""
    v = ALL[name]
    (smp,), _ = _restated(name, w, h)
    it, r2, Dx, Dy, eD = smp
    de = XD.de_of_x(it, r2, Dx, Dy, eD, v["max_iter"])
    worst, escaped, tried, left_out = 0.0, 0, 0, 0
    for p in range(0, w * h, stride):
        y, x = divmod(p, w)
        ei, ed = XD.exact_de_x(v, x, y, w, h)
        tried += 1
        if ei != it[y, x]:
            left_out += 1
            continue
        if ei < v["max_iter"]:
            escaped += 1
            assert ed > 0.0 and np.isfinite(de[y, x])
            worst = max(worst, abs(de[y, x] - ed) / ed)
        else:
            assert de[y, x] == 0.0
    print(f"{name}: {tried} tried, {left_out} left out, {escaped} escaped, worst |de - exact| / exact = {worst:.3g}")
    assert tried >= 30 and left_out == 0 and left_out <= 0.02 * tried
    assert escaped >= 10
    assert worst <= 1e-10, worst
    if name.startswith("tip"):                                    # every sample of the tip escapes, some 0.45 .. 24 px from the set
        assert (it < v["max_iter"]).all() and 0.1 < de.min() < de.max() < 100.0


# |de_bla - de_plain| / de_plain at 32 x 24, per view.  1e-10 unless the view's restatement, measured against exact_de_x on
# every pixel of this frame, is itself further than that from the exact derivative: then four times that measured error.  On D
# it is -- 651 escaped pixels, every iter equal to the exact one, worst |de - exact| / exact 3.28e-10 without the table and
# 2.09e-10 with it (the pixels nearest the set: the delta's own rounding over 3257 updates moves z, and D with it, whatever
# carries D) -- so D's bound is 4 * 3.28e-10.  T300: 2.63e-11 and 1.94e-11 against exact, the bound stays 1e-10.  The exact
# iteration is the yardstick; no GPU output entered these figures.
BLA_BOUND = {"D": 4 * 3.28e-10, "T300": 1e-10}


@pytest.mark.parametrize("name", ["D", "T300"])
def test_bla_agrees_with_plain_in_the_restatement(name):
    """32 x 24: iter with the extended table equals iter without it on at least 99.5 % of the pixels (the weakest agreement
    recorded for the family's flags is 0.99907), and on those de moves by rounding only: within BLA_BOUND relative.  Measured
    here: iter equal on every pixel of both views; worst |de_bla - de| / de 1.19e-10 on D, 9.7e-12 on T300."""
    v = ALL[name]
    w, h = 32, 24
    (p,), _ = _restated(name, w, h)
    (b,), counts = _restated(name, w, h, True)
    assert counts[1] > 0 and counts[2] > counts[0]
    same = p[0] == b[0]
    dp, db = XD.de_of_x(*p, v["max_iter"]), XD.de_of_x(*b, v["max_iter"])
    e = same & (p[0] < v["max_iter"])
    worst = float((np.abs(db[e] - dp[e]) / dp[e]).max())
    print(f"{name}: iter equal on {same.mean():.5f}, {int(e.sum())} escaped, worst |de_bla - de| / de = {worst:.3g}")
    assert same.mean() >= 0.995
    assert e.sum() >= 100 and worst <= BLA_BOUND[name], worst


def test_de_stays_finite_where_deriv_saturates():
    """view E: s ~ 1e-1003 and |dz/dc| ~ 1e1000 and more -- D crosses a double's range on its way, de is formed from the
    mantissas and comes out in pixel spacings; deriv at escape is back in range (|D| ~ 1 / de)"""
    v = ALL["E"]
    (smp,), _ = _restated("E", 48, 36)
    it, r2, Dx, Dy, eD = smp
    esc = it < v["max_iter"]
    de = XD.de_of_x(it, r2, Dx, Dy, eD, v["max_iter"])
    assert esc.sum() >= 100 and np.all(np.isfinite(de[esc])) and np.all(de[esc] > 0.0)
    assert np.all(np.isfinite(XD.deriv_of_x(it, Dx, Dy, eD, v["max_iter"])))
    sat = XD.deriv_of_x(np.zeros(2, np.int32), np.array([0.5, -0.5]), np.array([0.75, 0.5]), np.array([2000, -2000]), 1)
    assert np.array_equal(sat, [[np.inf, np.inf], [-0.0, 0.0]])
    far = XD.de_of_x(np.zeros(1, np.int32), np.array([16.0]), np.array([0.5]), np.array([0.0]), np.array([-3000]), 1)
    assert far[0] == np.inf                                       # beyond a double's range de saturates too, by the ldexp alone


# ---- kernels -------------------------------------------------------------------------------------------------------
# The kernels go by their blocks' names at the time (deep_isa.OLD_NAMES: DeepXDeArgs is DeepBlock<MandelFormula, true, true>).
# name -> (VGPRs at most, waves per SIMD at least, waves per SIMD of the kernel it extends, that kernel, SGPRs spilled at most).
# A 512-VGPR file in granules of 8 gives 4 waves up to 128 VGPRs and 3 up to 168: one wave less than the kernel each one
# extends (DeepXArgs 96 VGPRs and 5 waves, DeepXBlaArgs 127 and 4).  Measured: 106 VGPRs and 4 waves, 144 and 3.
# No scratch and no VGPR spill.  SGPRs are another matter: every deep kernel sits at the cap of 106 SGPRs and parks kernel
# arguments of its colour stage in VGPR lanes (v_writelane in the prologue, v_readlane where they are used) -- 76 of them in
# DeepXArgs, 78 in DeepXBlaArgs.  The derivative's block adds nine scalars (sm, es, two plane pointers, shade,
# edge_px) and the two new kernels park 84 and 87: that is the bound here, with at most nine more than the kernel each extends.
# What matters for time is where they are read back: not inside the orbit loop (test below, on the ISA).
BUDGET = {"DeepXDeArgs": (128, 4, 5, "DeepXArgs", 84), "DeepXDeBlaArgs": (168, 3, 4, "DeepXBlaArgs", 87)}
SGPR_SPILL_OVER_PARENT = 9


@pytest.fixture(scope="module")
def device_build():
    return deep_isa.by_old_name() or pytest.skip("hipcc not available")


def test_deepx_de_kernels_keep_their_register_budget(fr, device_build):
    for name, (max_vgpr, min_occ, parent_occ, parent, max_sspill) in BUDGET.items():
        u, pu = device_build[name].usage, device_build[parent].usage
        print(name, u, "extends", parent, pu)
        assert u["ScratchSize [bytes/lane]"] == 0 and u.get("VGPRs Spill", 0) == 0, (name, u)
        assert u["VGPRs"] <= max_vgpr and u["Occupancy [waves/SIMD]"] >= min_occ, (name, u)
        assert pu["Occupancy [waves/SIMD]"] == parent_occ and u["Occupancy [waves/SIMD]"] >= parent_occ - 1, (name, u, pu)
        assert u["SGPRs Spill"] <= max_sspill, (name, u)
        assert u["SGPRs Spill"] <= pu["SGPRs Spill"] + SGPR_SPILL_OVER_PARENT, (name, u, pu)


def _loops(body):
    """the instructions of a kernel's assembly and its loops as (first, last) instruction of every backward branch's range"""
    labels, ins = {}, []
    for line in body:
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        t = line.strip()
        if t and t[0] not in ";.":
            ins.append(t)
    loops = []
    for i, t in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", t)
        if m and labels.get(m.group(1), i + 1) <= i:
            loops.append((labels[m.group(1)], i))
    return ins, loops


def test_the_orbit_loop_reads_back_no_spilled_sgpr(device_build):
    """On the ISA of the two kernels: the orbit loop -- the smallest loop that holds every fp64 multiply of the kernel's loops,
    both modes' steps and the derivative's -- has no v_readlane, no v_writelane and no scratch access.  The parked SGPRs are
    written once in the prologue and read back per sample, in the colour stage around the loop.  Measured: loops of 822 and
    1030 instructions with 96 and 113 fp64 multiplies, 47 and 60 v_ldexp_f64; 16 and 17 v_readlane per sample outside them."""
    for name in BUDGET:
        ins, loops = _loops(device_build[name].asm)
        count = lambda a, b, pat: sum(1 for t in ins[a:b + 1] if re.match(pat, t))
        mul = "v_mul_f64|v_fma_f64"
        most = max(count(a, b, mul) for a, b in loops)
        assert most >= 40, (name, most)                            # two modes' steps and the derivative: 96 and 113 measured
        a, b = min((l for l in loops if count(*l, mul) == most), key=lambda l: l[1] - l[0])
        assert count(a, b, "v_ldexp_f64") >= 20, name               # it is the extended loop
        print(name, "orbit loop", b - a + 1, "instructions,", most, "fp64 multiplies,", count(a, b, "v_ldexp_f64"), "ldexp;",
              "v_readlane in the kernel", count(0, len(ins), "v_readlane"), "v_writelane", count(0, len(ins), "v_writelane"))
        assert count(a, b, "v_readlane|v_writelane") == 0, name
        assert count(a, b, "scratch_|buffer_load|buffer_store") == 0, name
        assert count(0, len(ins), "v_writelane") > 0                 # the spills are there, outside
