"""Distance estimates for deep Mandelbrot views (fr_render_deep_de): the parts that need no GPU -- the ABI, validation, the
Python wrapper, the restatement (tests/deep_de_ref.py) against the plain and BLA restatements it extends and against the
direct iteration of z^2 + c and its derivative in Python integers, and the register budget of the kernels."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import deep_bla_ref as BR
import deep_isa
import deep_de_ref as D
import deep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 48, 36


def _view(fr, cx="-0.5", cy="0", frac_bits=0, reserved=0):
    return fr._capi.fr_deep_view(cx.encode() if isinstance(cx, str) else cx, cy.encode() if isinstance(cy, str) else cy,
                                 frac_bits, reserved)


# ---- ABI -----------------------------------------------------------------------------------------------------------
def test_abi_layout_symbols_and_defaults(fr, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "fractalrenderer_amd.h")).read()
    assert re.search(r"#define FR_HAS_DEEP_DE 1", hdr)
    for name in ("fr_deep_de_default", "fr_deep_de_validate", "fr_render_deep_de", "fr_render_deep_de_async"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in fr._capi.SIGNATURES and hasattr(fr.lib(), name), name
    mirror = fr._capi.fr_deep_de
    assert C.sizeof(mirror) == 24
    assert [(f, getattr(mirror, f).offset) for f, _ in mirror._fields_] == [("de", 0), ("deriv", 8), ("shade", 16), ("edge_px", 20)]
    gcc = shutil.which("gcc")
    if gcc:                                                       # the C compiler's view of the same struct
        src = tmp_path / "layout.c"
        src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"fractalrenderer_amd.h\"\n"
                       "#if !defined(FR_HAS_DEEP_DE) || FR_HAS_DEEP_DE != 1\n#error FR_HAS_DEEP_DE\n#endif\n"
                       "int main(void) { printf(\"%zu %zu %zu %zu %zu\\n\", sizeof(fr_deep_de), offsetof(fr_deep_de, de), "
                       "offsetof(fr_deep_de, deriv), offsetof(fr_deep_de, shade), offsetof(fr_deep_de, edge_px)); return 0; }\n")
        exe = tmp_path / "layout"
        subprocess.run([gcc, "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["24", "0", "8", "16", "20"]
    e = mirror(1, 2, 7, 9.0)
    assert fr.lib().fr_deep_de_default(C.byref(e)) == 0
    assert (e.de, e.deriv, e.shade) == (None, None, 0) and e.edge_px == np.float32(1.8)
    assert fr.lib().fr_deep_de_default(None) == fr._capi.FR_ERR_INVALID_ARG
    # 0.005 c-plane units (the debug shader's edge) at zoom 3.0 on 1080 rows, in pixel spacings
    assert abs(0.005 / (3.0 / 1080) - 1.8) < 1e-12
    assert fr.DEEP_DE_EDGE_PX == 1.8 and "DEEP_DE_EDGE_PX" in fr.__all__


# ---- validation ----------------------------------------------------------------------------------------------------
def test_validation_matrix(fr):
    F = fr._capi
    L = fr.lib()
    L.fr_deep_validate.restype = C.c_int
    L.fr_deep_validate.argtypes = [C.POINTER(F.fr_params), C.POINTER(F.fr_deep_view), C.c_uint32, C.c_uint32]
    good = _view(fr, R.VIEW_A["cx"], R.VIEW_A["cy"])
    plane = np.zeros(4, np.float64)

    def params(**kw):
        p = fr.FractalState(zoom=1e-30).to_params(fr.FractalType.Mandelbrot, fr.Precision.F64)
        for k, val in kw.items():
            setattr(p, k, val)
        return p

    def check(W=64, H=48, view=good, de=None, **kw):
        p = params(**kw)
        e = de if de is not None else F.fr_deep_de(plane.ctypes.data, None, 0, 1.8)
        return L.fr_deep_de_validate(C.byref(p), C.byref(view), C.byref(e), W, H), L.fr_deep_validate(C.byref(p), C.byref(view), W, H)

    assert check() == (F.FR_OK, F.FR_OK)
    assert check(flags=F.FR_FLAG_DEEP_BLA | F.FR_FLAG_POST_CHAIN) == (F.FR_OK, F.FR_OK)
    # every case fr_deep_validate refuses is refused here, with its status
    unsupported = [dict(fractal_type=t) for t in (1, 2, 3, 4, 5, 99)] + [dict(precision=0), dict(orbit_trap_enabled=1),
                   dict(stripe_enabled=1), dict(interior_style=2), dict(flags=F.FR_FLAG_DEEP_JULIA_BLA),
                   dict(flags=F.FR_FLAG_DEEPX_JULIA_BLA), dict(flags=F.FR_FLAG_DEEP_BLA | F.FR_FLAG_DEEP_JULIA_BLA)]
    for kw in unsupported:
        assert check(**kw) == (F.FR_ERR_UNSUPPORTED, F.FR_ERR_UNSUPPORTED), kw
    invalid = [dict(W=0), dict(H=0), dict(W=65536, H=32768), dict(max_iterations=0), dict(max_iterations=(1 << 24) + 1),
               dict(antialiasing_samples=17), dict(antialiasing_samples=-1), dict(bailout=0.0), dict(bailout=float("nan")),
               dict(bailout=65537.0), dict(zoom=1e-291), dict(zoom=1001.0), dict(zoom=-1e-30), dict(zoom=0.0),
               dict(julia_c_real=float("inf")), dict(view=_view(fr, "1e", "0")), dict(view=_view(fr, "0", "0", 0, 3)),
               dict(view=_view(fr, "0", "0", 100)), dict(view=_view(fr, "1" * 4097, "0")), dict(view=_view(fr, None, "0"))]
    for kw in invalid:
        assert check(**kw) == (F.FR_ERR_INVALID_ARG, F.FR_ERR_INVALID_ARG), kw
    assert check(center_x=float("nan"), center_y=float("inf"), interior_style=1) == (F.FR_OK, F.FR_OK)
    # its own rules
    p = params()
    assert L.fr_deep_de_validate(C.byref(p), C.byref(good), None, 64, 48) == F.FR_ERR_INVALID_ARG
    assert L.fr_deep_de_validate(None, C.byref(good), C.byref(F.fr_deep_de(None, None, 0, 1.8)), 64, 48) == F.FR_ERR_INVALID_ARG
    assert L.fr_deep_de_validate(C.byref(p), None, C.byref(F.fr_deep_de(None, None, 0, 1.8)), 64, 48) == F.FR_ERR_INVALID_ARG
    for shade in (2, -1, 256):
        assert check(de=F.fr_deep_de(None, None, shade, 1.8))[0] == F.FR_ERR_INVALID_ARG, shade
    for edge in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert check(de=F.fr_deep_de(None, None, 1, edge))[0] == F.FR_ERR_INVALID_ARG, edge
        assert check(de=F.fr_deep_de(None, None, 0, edge))[0] == F.FR_OK, edge      # not read without the shading
    assert check(de=F.fr_deep_de(None, None, 1, 1e-30))[0] == F.FR_OK
    assert check(de=F.fr_deep_de(None, None, 1, 0.25))[0] == F.FR_OK               # the planes are the render's business
    # the render entry points: a NULL context, params, view or de is an invalid argument
    o = F.fr_output(None, None, None, F.FR_MEM_HOST, 0)
    e = F.fr_deep_de(plane.ctypes.data, None, 0, 1.8)
    assert L.fr_render_deep_de(None, C.byref(p), C.byref(good), C.byref(e), 64, 48, None, C.byref(o)) == F.FR_ERR_INVALID_ARG
    assert L.fr_render_deep_de_async(None, C.byref(p), C.byref(good), C.byref(e), 64, 48, None, C.byref(o), None) \
        == F.FR_ERR_INVALID_ARG


# ---- the Python wrapper ----------------------------------------------------------------------------------------------
def test_python_wrapper_signature_flags_and_the_value_error(fr):
    sig = inspect.signature(fr.Renderer.render_deep_de)
    names = list(sig.parameters)
    assert names == ["self", "state", "width", "height", "view", "post_chain", "rgba", "nu", "iter", "de", "deriv", "shade",
                     "edge_px", "shard", "stream", "sync", "bla"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["view"], d["post_chain"], d["shade"], d["edge_px"], d["sync"], d["bla"]) == (None, False, False, 1.8, True, False)
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names[5:])

    class Ctx:                                                    # a renderer without a context: the calls it would make
        calls = []

        class _lib:
            @staticmethod
            def fr_render_deep_de(ctx, p, v, e, w, h, sh, out):
                Ctx.calls.append(("sync", p._obj.flags, p._obj.fractal_type, p._obj.precision, e._obj.shade, e._obj.edge_px,
                                  e._obj.de, e._obj.deriv, out._obj.memory, out._obj.rgba))
                return 0

            @staticmethod
            def fr_render_deep_de_async(ctx, p, v, e, w, h, sh, out, stream):
                Ctx.calls.append(("async", p._obj.flags, stream.value))
                return 0
        _ctx = None
        _output = fr.Renderer._output
        _ptr = staticmethod(fr.Renderer._ptr)

    st = fr.FractalState(zoom=1e-30)
    de = np.zeros((4, 6), np.float64)
    deriv = np.zeros((4, 6, 2), np.float64)
    call = fr.Renderer.render_deep_de
    ctx = Ctx()
    call(ctx, st, 6, 4, fr.DeepView("0", "0"), de=de)
    call(ctx, st, 6, 4, de=de, deriv=deriv, shade=True, edge_px=0.25, bla=True, post_chain=True)
    call(ctx, st, 6, 4, de=de, sync=False, stream=77, bla=True)
    F = fr._capi
    assert Ctx.calls[0] == ("sync", 0, 0, F.FR_PRECISION_F64, 0, np.float32(1.8), de.ctypes.data, None, F.FR_MEM_HOST, None)
    assert Ctx.calls[1][:6] == ("sync", F.FR_FLAG_DEEP_BLA | F.FR_FLAG_POST_CHAIN, 0, F.FR_PRECISION_F64, 1, 0.25)
    assert Ctx.calls[1][6:8] == (de.ctypes.data, deriv.ctypes.data)
    assert Ctx.calls[2] == ("async", F.FR_FLAG_DEEP_BLA, 77)
    with pytest.raises(ValueError):
        call(ctx, st, 6, 4, fr.DeepView("0", "0", zoom="1e-400"), de=de)
    with pytest.raises(ValueError):
        call(ctx, st, 6, 4, de=np.zeros((4, 6), np.float32))
    with pytest.raises(ValueError):
        call(ctx, st, 6, 4, de=de, deriv=np.zeros((4, 6), np.float64))
    with pytest.raises(ValueError):
        call(ctx, st, 6, 4, de=de, stream=5)
    assert len(Ctx.calls) == 3


# ---- the restatement -------------------------------------------------------------------------------------------------
CPU_VIEWS = {"A": R.VIEW_A, "B": R.VIEW_B, "tip": D.TIP}


@pytest.mark.parametrize("name", ["shallow", "A", "B", "tip"])
def test_planes_do_not_depend_on_the_derivative(name):
    """(iter, r2) of the restatement are deep_ref.perturb's without a table and deep_bla_ref.perturb_bla's with one, bit for
    bit, and so are the step counts"""
    v = dict(CPU_VIEWS, shallow=R.SHALLOW)[name]
    orb = R.reference_orbit(v["cx"], v["cy"], v["zoom"], v["max_iter"])
    dcx, dcy = R.sample_dc(W, H, v["zoom"], 1, 0)
    s = D.spacing(v["zoom"], H)
    it, r2, Dx, Dy, _ = D.perturb_de(orb, dcx, dcy, v["max_iter"], [], s)
    pit, pr2, _ = R.perturb(orb, dcx, dcy, v["max_iter"])
    assert np.array_equal(it, pit) and np.array_equal(r2.view(np.uint64), pr2.view(np.uint64))
    tab = BR.bla_table(orb, BR.dcmax(W, H, v["zoom"]))
    it, r2, Dx, Dy, counts = D.perturb_de(orb, dcx, dcy, v["max_iter"], tab, s)
    bit, br2, bcounts = BR.perturb_bla(orb, dcx, dcy, v["max_iter"], tab)
    assert np.array_equal(it, bit) and np.array_equal(r2.view(np.uint64), br2.view(np.uint64)) and counts == bcounts
    if name != "shallow":
        assert counts[1] > 0


def test_first_update_and_interior():
    """D' = (s, 0) exactly after the first update, whatever the sample; interior samples have de 0 and deriv (0, 0)"""
    v = dict(R.VIEW_A, max_iter=1)
    (smp,), _ = D.restate_de(v, W, H, bailout=1e-3)               # every sample escapes at once
    it, r2, Dx, Dy = smp
    assert np.all(it == 0) and np.all(Dx == D.spacing(v["zoom"], H)) and np.all(Dy == 0.0)
    (smp,), _ = D.restate_de(v, W, H)                            # none does
    it, r2, Dx, Dy = smp
    assert np.all(it == 1) and not D.de_of(it, r2, Dx, Dy, 1).any() and not D.deriv_of(it, Dx, Dy, 1).any()


@pytest.mark.parametrize("name,stride", [("A", 1), ("B", 3), ("tip", 4)])
def test_restatement_agrees_with_the_exact_derivative(name, stride):
    """The restatement against exact_de (z^2 + c and d <- 2 z d + 1 in Python integers at F + 64 fraction bits) at 48 x 36: on
    every pixel of A, every third of B, every fourth of the tip at 1e-290.  No pixel is left out for a differing iter (0
    differ on all three), and |de - exact| / exact <= 1e-10.  Measured here, restatement against exact: A 3.1e-12,
    B 1.0e-11 (5.9e-12 with another choice of every third pixel), tip 1.8e-15; the bound is about ten times the worst."""
    v = CPU_VIEWS[name]
    (smp,), _ = D.restate_de(v, W, H)
    it, r2, Dx, Dy = smp
    de = D.de_of(it, r2, Dx, Dy, v["max_iter"])
    worst, escaped = 0.0, 0
    for p in range(0, W * H, stride):
        y, x = divmod(p, W)
        ei, ed = D.exact_de(v["cx"], v["cy"], x, y, W, H, v["zoom"], v["max_iter"])
        assert ei == it[y, x], (x, y, ei, int(it[y, x]))
        if ei < v["max_iter"]:
            escaped += 1
            assert ed > 0.0
            worst = max(worst, abs(de[y, x] - ed) / ed)
        else:
            assert de[y, x] == 0.0
    print(f"{name}: {escaped} escaped, worst |de - exact| / exact = {worst:.3g}")
    assert escaped >= 100
    assert worst <= 1e-10, worst


@pytest.mark.parametrize("name,w,h", [("A", W, H), ("B", W, H), ("C", 32, 24), ("tip", W, H)])
def test_bla_agrees_with_plain_in_the_restatement(name, w, h):
    """iter with the table equals iter without it on every pixel (measured: 1.0 on A, B, C at 32 x 24 and the tip), and a BLA
    step's derivative is that of the map it applies: de moves by rounding only (measured: at most 5.5e-12 relative on A, B
    and the tip, where the exact derivative is 1e-11 away)"""
    v = dict(CPU_VIEWS, C=BR.VIEW_C)[name]
    orb = R.reference_orbit(v["cx"], v["cy"], v["zoom"], v["max_iter"])
    (p,), _ = D.restate_de(v, w, h, orbit=orb)
    (b,), counts = D.restate_de(v, w, h, orbit=orb, bla=True)
    assert counts[1] > 0
    assert np.array_equal(p[0], b[0])
    if name != "C":                                               # C: filaments 0.005 pixels away, de is noise there
        dp, db = D.de_of(*p, v["max_iter"]), D.de_of(*b, v["max_iter"])
        e = p[0] < v["max_iter"]
        assert (np.abs(db[e] - dp[e]) / dp[e]).max() <= 1e-10


def test_view_c_is_why():
    """the median escaped pixel of view C lies 0.005 pixel spacings from the set"""
    v = BR.VIEW_C
    (p,), _ = D.restate_de(v, 32, 24, bla=True)
    de = D.de_of(*p, v["max_iter"])
    assert 0.002 <= np.median(de[p[0] < v["max_iter"]]) <= 0.01


def test_shading_restated():
    f = np.float32
    rgb = np.array([[1.0, 0.5, 0.25]] * 5, f)
    de = np.array([0.0, 0.9, 1.8, 5.0, -3.0])
    esc = np.array([True, True, True, True, True])
    out = D.shade(rgb, de, esc, 1.8)
    assert np.array_equal(out[2], rgb[2]) and np.array_equal(out[3], rgb[3])           # at and past the edge: untouched
    dark = rgb[0] * (f(1.0) - f(0.3)) + (rgb[0] * f(0.7)) * f(0.3)                     # on the set: t = 0.3
    assert np.array_equal(out[0], dark) and np.array_equal(out[4], dark)
    assert np.all(out[1] < rgb[1]) and np.all(out[1] > dark)
    assert np.array_equal(D.shade(rgb, de, ~esc, 1.8), rgb)                             # interior samples are not shaded


# ---- kernels -------------------------------------------------------------------------------------------------------
# (VGPRs, SGPRs, scratch bytes per lane, waves per SIMD) of every deep_kernel and level kernel of the parent commit, read from
# its build with -Rpass-analysis=kernel-resource-usage, under the blocks' names at the time (deep_isa.OLD_NAMES)
PARENT = {
    "DeepArgs": (83, 106, 0, 5), "DeepBlaArgs": (113, 106, 0, 4), "DeepXArgs": (96, 106, 0, 5), "DeepXBlaArgs": (127, 106, 0, 4),
    "DeepShipArgs": (89, 106, 0, 5), "DeepShipBlaArgs": (120, 106, 0, 4), "DeepShipXArgs": (101, 106, 0, 4),
    "DeepShipXBlaArgs": (130, 106, 0, 3), "DeepJuliaArgs": (87, 106, 0, 5), "DeepJuliaBlaArgs": (115, 106, 0, 4),
    "DeepJuliaXArgs": (93, 106, 0, 5), "DeepJuliaXBlaArgs": (126, 106, 0, 4),
    "deep_bla_level_kernel": (40, 34, 0, 8), "deepx_bla_level_kernel": (53, 38, 0, 8), "deep_ship_bla_level_kernel": (59, 38, 0, 8),
    "deepx_ship_bla_level_kernel": (68, 38, 0, 7), "deep_julia_bla_level_kernel": (32, 30, 0, 8),
    "deepx_julia_bla_level_kernel": (42, 32, 0, 8),
}
# the new instantiations: at most this many VGPRs, at least this many waves per SIMD -- the occupancy of the kernel each one
# extends (DeepArgs 5, DeepBlaArgs 4); measured 94 and 123 VGPRs
BUDGET = {"DeepDeArgs": (96, 5), "DeepDeBlaArgs": (128, 4)}


def test_deep_kernels_keep_their_register_budget(fr):
    built = deep_isa.by_old_name()
    if built is None:
        pytest.skip("hipcc not available")
    usage = {name: k.usage for name, k in built.items()}
    # all twenty deep_kernel instantiations and the six level kernels, and nothing else
    assert set(deep_isa.kernels()) == set(deep_isa.OLD_NAMES.values()) | deep_isa.LEVEL_KERNELS and len(usage) == 26
    for name, want in PARENT.items():
        u = usage[name]
        got = (u["VGPRs"], u["TotalSGPRs"], u["ScratchSize [bytes/lane]"], u["Occupancy [waves/SIMD]"])
        assert got == want and u.get("VGPRs Spill", 0) == 0, (name, got, want)
    for name, (max_vgpr, min_occ) in BUDGET.items():
        u = usage[name]
        assert u["ScratchSize [bytes/lane]"] == 0 and u.get("VGPRs Spill", 0) == 0, (name, u)
        assert u["VGPRs"] <= max_vgpr and u["Occupancy [waves/SIMD]"] >= min_occ, (name, u)
