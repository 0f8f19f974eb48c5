"""Deep Phoenix views below 1e-290 with bilinear approximation (FR_FLAG_DEEPX_PHOENIX_BLA): the parts that need no GPU -- the ABI, the
validation, the Python wrapper, and the restatement (tests/deepx_phoenix_bla_ref.py) against the unflagged restatement and the
recorded exact fixed-point frames, what it skips, and the shape of its table.

Measured with the restatement at 24 x 18, aa 1 (iter differing from the unflagged restatement / from the exact frame, of 432):
PX310 0 / 0, PX400A 0 / 0, PX400B 0 / 0, PXRET 0 / 0, TIP1000 0 / 0 (the unflagged restatement: 0 from exact as well)."""
import ctypes as C
import functools
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import deepx_phoenix_bla_ref as XB
import deepx_phoenix_ref as PX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = PX.GOLDEN_SIZE              # 24 x 18
DEEP = ("PX310", "PX400A", "PX400B", "PXRET", "TIP1000")

# [single steps, BLA steps, updates skipped] of the restatement at 24 x 18, aa 1: taken from the restatement (never from a
# device), so that a change of the rule or of its restatement shows
PINNED = {
    "PX310": (229228, 1409, 889774),
    "PX400A": (238009, 2371, 1165248),
    "PX400B": (297560, 2795, 1923148),
    "PXRET": (308980, 2450, 946162),
    "TIP1000": (29247, 2171, 707530),
    "NUC201X": (864, 2592, 1041120),
}


@functools.lru_cache(maxsize=None)
def _orbit(name):
    return PX.orbit_of(XB.VIEWS[name])


@functools.lru_cache(maxsize=None)
def _flagged(name):
    """computed once per view, shared, never changed"""
    (planes,), counts = XB.samples_x_bla(XB.VIEWS[name], W, H, orbit=_orbit(name))
    return planes, tuple(counts)


@functools.lru_cache(maxsize=None)
def _unflagged(name):
    return PX.samples_x(XB.VIEWS[name], W, H, orbit=_orbit(name))[0]


def _updates(it, max_iter):
    return int(np.where(it < max_iter, it.astype(np.int64) + 1, max_iter).sum())


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_flag_counts_and_table_are_in_the_header_and_capi(fr, tmp_path):
    K = fr._capi
    hdr = open(os.path.join(ROOT, "include", "fractalrenderer_amd.h")).read()
    assert re.search(r"#define FR_FLAG_DEEPX_PHOENIX_BLA\s+0x100u", hdr)
    assert re.search(r"#define FR_HAS_DEEPX_PHOENIX_BLA 1", hdr)
    assert re.search(r"int fr_ctx_last_deepx_phoenix_steps\(fr_ctx\* ctx, uint64_t out\[3\]\);", hdr)
    assert "the extended path has no table" not in hdr and "Out of scope: BLA for extended Phoenix views" not in hdr
    internal = open(os.path.join(ROOT, "fractalrenderer_amd", "csrc", "fr_internal.h")).read()
    assert re.search(r"int64_t fr_deepx_phoenix_bla_table\(fr_ctx\* ctx, void\* r, double\* mb, int32_t\* mb_exp, int64_t n\);",
                     internal)
    assert K.FR_FLAG_DEEPX_PHOENIX_BLA == 0x100 == fr.FR_FLAG_DEEPX_PHOENIX_BLA
    assert "FR_FLAG_DEEPX_PHOENIX_BLA" in fr.__all__
    assert "fr_ctx_last_deepx_phoenix_steps" in K.SIGNATURES
    assert "fr_deepx_phoenix_bla_table" in K.INTERNAL_SIGNATURES
    assert hasattr(fr.lib(), "fr_ctx_last_deepx_phoenix_steps") and hasattr(fr.lib(), "fr_deepx_phoenix_bla_table")
    assert inspect.signature(fr.Renderer.render_deepx_phoenix).parameters["xbla"].default is False
    assert callable(fr.Renderer.last_deepx_phoenix_steps)
    flags = (K.FR_FLAG_POST_CHAIN, fr.FR_FLAG_DEEP_BLA, fr.FR_FLAG_DEEPX_BLA, fr.FR_FLAG_DEEP_SHIP_BLA, fr.FR_FLAG_DEEPX_SHIP_BLA,
             fr.FR_FLAG_DEEP_JULIA_BLA, fr.FR_FLAG_DEEPX_JULIA_BLA, fr.FR_FLAG_DEEP_PHOENIX_BLA, fr.FR_FLAG_DEEPX_PHOENIX_BLA)
    assert sorted(flags) == [1, 2, 4, 8, 16, 32, 64, 128, 256]
    assert fr.lib().fr_ctx_last_deepx_phoenix_steps(None, (C.c_uint64 * 3)()) == K.FR_ERR_INVALID_ARG
    assert fr.lib().fr_deepx_phoenix_bla_table(None, None, None, None, 0) == K.FR_ERR_INVALID_ARG
    gcc = shutil.which("gcc")
    if gcc:
        src = tmp_path / "macros.c"
        src.write_text("#include \"fractalrenderer_amd.h\"\n"
                       "#if !defined(FR_HAS_DEEPX_PHOENIX_BLA) || FR_HAS_DEEPX_PHOENIX_BLA != 1\n#error FR_HAS_DEEPX_PHOENIX_BLA\n#endif\n"
                       "#if FR_FLAG_DEEPX_PHOENIX_BLA != 0x100u\n#error flag value\n#endif\n"
                       "#if (FR_FLAG_DEEPX_PHOENIX_BLA & (FR_FLAG_POST_CHAIN | FR_FLAG_DEEP_BLA | FR_FLAG_DEEPX_BLA | "
                       "FR_FLAG_DEEP_SHIP_BLA | FR_FLAG_DEEPX_SHIP_BLA | FR_FLAG_DEEP_JULIA_BLA | FR_FLAG_DEEPX_JULIA_BLA | "
                       "FR_FLAG_DEEP_PHOENIX_BLA)) != 0\n"
                       "#error flag bits overlap\n#endif\n"
                       "int (*a)(fr_ctx*, uint64_t[3]) = fr_ctx_last_deepx_phoenix_steps;\n")
        subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "macros.o")], check=True)


def test_the_wrapper_sets_exactly_that_flag(fr):
    seen = {}

    class Probe(fr.Renderer):
        def __init__(self):
            self._lib = fr.lib()

        def _render_call(self, fn_sync, fn_async, params, *a):
            seen["flags"] = params[0]._obj.flags
            seen["entry"] = fn_sync is self._lib.fr_render_deepx_phoenix and fn_async is self._lib.fr_render_deepx_phoenix_async

    r = Probe()
    st = fr.FractalState(max_iterations=64)
    view = fr.DeepView("0.1", "0.2", zoom="1e-400")
    r.render_deepx_phoenix(st, 8, 8, view, fr.PhoenixParams(), xbla=True)
    assert seen == {"flags": fr.FR_FLAG_DEEPX_PHOENIX_BLA, "entry": True}
    r.render_deepx_phoenix(st, 8, 8, view, fr.PhoenixParams(), xbla=True, post_chain=True)
    assert seen == {"flags": fr.FR_FLAG_DEEPX_PHOENIX_BLA | fr._capi.FR_FLAG_POST_CHAIN, "entry": True}
    r.render_deepx_phoenix(st, 8, 8, view, fr.PhoenixParams())
    assert seen == {"flags": 0, "entry": True}
    # no other wrapper knows the flag: render_deep_phoenix's bla is FR_FLAG_DEEP_PHOENIX_BLA
    seen.clear()
    Probe._render_call = lambda self, fn_sync, fn_async, params, *a: seen.update(flags=params[0]._obj.flags)
    r.render_deep_phoenix(fr.FractalState(zoom=1e-30, max_iterations=64), 8, 8, fr.DeepView("0.1", "0.2"), fr.PhoenixParams(), bla=True)
    assert seen == {"flags": fr.FR_FLAG_DEEP_PHOENIX_BLA}
    assert "xbla" not in inspect.signature(fr.Renderer.render_deep_phoenix).parameters


# ---- validation ------------------------------------------------------------------------------------------------------------
def test_validators(fr):
    """fr_deepx_phoenix_validate accepts its flag, alone or with the post chain, and keeps refusing the seven older BLA flags, alone
    or next to it; every other deep validator refuses 0x100"""
    L, K = fr.lib(), fr._capi
    U = K.FR_ERR_UNSUPPORTED
    own = K.FR_FLAG_DEEPX_PHOENIX_BLA
    old = (K.FR_FLAG_DEEP_BLA, K.FR_FLAG_DEEPX_BLA, K.FR_FLAG_DEEP_SHIP_BLA, K.FR_FLAG_DEEPX_SHIP_BLA, K.FR_FLAG_DEEP_JULIA_BLA,
           K.FR_FLAG_DEEPX_JULIA_BLA, K.FR_FLAG_DEEP_PHOENIX_BLA)
    ph = fr.PhoenixParams().to_c()
    dv = K.fr_deep_view(b"0.1", b"0.2", 0, 0)
    xv = K.fr_deepx_view(b"0.1", b"0.2", b"1e-400", 0, 0)

    def check(fn, view, flags, ftype=fr.FractalType.Phoenix):
        p = fr.FractalState(zoom=1e-30, max_iterations=64).to_params(ftype, fr.Precision.F64, False)
        p.flags |= flags
        st = fn(C.byref(p), C.byref(ph), C.byref(view), 8, 8)
        return st, (L.fr_last_error() or b"").decode() if st else ""

    deep, deepx = L.fr_deep_phoenix_validate, L.fr_deepx_phoenix_validate
    assert check(deepx, xv, 0)[0] == 0 and check(deepx, xv, own)[0] == 0 and check(deepx, xv, own | K.FR_FLAG_POST_CHAIN)[0] == 0
    for f in old:
        for flags in (f, f | own):
            st, msg = check(deepx, xv, flags)
            assert st == U and "BLA" in msg, (flags, msg)
    assert check(deepx, xv, own, fr.FractalType.Mandelbrot)[0] == U       # the other rules of the path hold with the flag
    # fr_deep_phoenix_validate: its own flag still, 0x100 never
    assert check(deep, dv, K.FR_FLAG_DEEP_PHOENIX_BLA)[0] == 0
    for flags in (own, own | K.FR_FLAG_POST_CHAIN, own | K.FR_FLAG_DEEP_PHOENIX_BLA):
        st, msg = check(deep, dv, flags)
        assert st == U and "FR_FLAG_DEEPX_PHOENIX_BLA" in msg, (flags, msg)

    # the six validators of the other deep paths, each with its own flag too
    def plain(fn, view, ftype, flags, zoom=1e-30):
        p = fr.FractalState(zoom=zoom, max_iterations=64).to_params(ftype, fr.Precision.F64, False)
        p.flags |= flags
        return fn(C.byref(p), C.byref(view), 8, 8)

    T = fr.FractalType
    for fn, view, ftype, mine in ((L.fr_deep_validate, dv, T.Mandelbrot, K.FR_FLAG_DEEP_BLA),
                                  (L.fr_deepx_validate, xv, T.Mandelbrot, K.FR_FLAG_DEEPX_BLA),
                                  (L.fr_deep_ship_validate, dv, T.BurningShip, K.FR_FLAG_DEEP_SHIP_BLA),
                                  (L.fr_deepx_ship_validate, xv, T.BurningShip, K.FR_FLAG_DEEPX_SHIP_BLA),
                                  (L.fr_deep_julia_validate, dv, T.JuliaSet, K.FR_FLAG_DEEP_JULIA_BLA),
                                  (L.fr_deepx_julia_validate, xv, T.JuliaSet, K.FR_FLAG_DEEPX_JULIA_BLA)):
        assert plain(fn, view, ftype, 0) == 0 and plain(fn, view, ftype, mine) == 0, fn
        assert plain(fn, view, ftype, own) == U and plain(fn, view, ftype, own | mine) == U, fn
        assert "FR_FLAG_DEEPX_PHOENIX_BLA" in (L.fr_last_error() or b"").decode()


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["PX310", "PX400A", "PX400B", "PXRET"])
def test_iter_equals_the_unflagged_restatement_and_the_exact_frame(name):
    """24 x 18: on every pixel of the four views (0 differences measured, so nothing is capped)"""
    v = XB.VIEWS[name]
    (it, _, _, _), counts = _flagged(name)
    pit = _unflagged(name)[0]
    ex = PX.exact_golden()[name]
    print(name, "differs from unflagged", int((it != pit).sum()), "from exact", int((it != ex).sum()), "counts", counts)
    assert np.array_equal(it, pit), int((it != pit).sum())
    assert np.array_equal(it, ex), int((it != ex).sum())
    assert counts[1] > 0
    assert counts[0] + counts[2] == _updates(pit, v["max_iter"])


def test_tip1000_against_the_unflagged_restatement_and_the_exact_frame():
    """escapes on margins of 1e-1000 at |z|^2 = 4: the counts the module's docstring reports, measured 0 / 0 / 0"""
    v = XB.VIEWS["TIP1000"]
    (it, _, _, _), counts = _flagged("TIP1000")
    pit = _unflagged("TIP1000")[0]
    ex = PX.exact_golden()["TIP1000"]
    d = (int((it != pit).sum()), int((it != ex).sum()), int((pit != ex).sum()))
    print("TIP1000 flagged != unflagged, flagged != exact, unflagged != exact:", d, "counts", counts)
    assert d == (0, 0, 0)
    assert counts[1] > 0
    assert counts[0] + counts[2] == _updates(pit, v["max_iter"])


@pytest.mark.parametrize("name", list(PINNED))
def test_what_the_restatement_skips_is_pinned(name):
    v = XB.VIEWS[name]
    (it, _, _, _), counts = _flagged(name)
    print(name, "N", len(_orbit(name)[1]) - 1, "counts", counts)
    assert counts == PINNED[name]
    assert counts[1] > 0
    if np.array_equal(it, _unflagged(name)[0]):
        assert counts[0] + counts[2] == _updates(it, v["max_iter"])      # every update is a single step or skipped


def test_one_recorded_exact_frame_is_recomputed_on_a_sample_of_pixels():
    """the fixture the comparisons above lean on: PX310's exact frame on a diagonal of its pixels"""
    ex = PX.exact_golden()["PX310"]
    for x, y in ((0, 0), (5, 4), (11, 9), (17, 13), (23, 17)):
        assert PX.exact_iter_x(PX.PX310, x, y, W, H) == ex[y, x], (x, y)


def test_nuc201x_is_interior_and_needs_the_extended_radius():
    """every pixel is interior, and the loop trips are below a tenth of what the table takes with the single step's radius rounded
    through a double (the orbit returns to 2^-1312 once per period; 2^-54 |a| underflows there)"""
    v = XB.VIEWS["NUC201X"]
    (it, _, _, _), counts = _flagged("NUC201X")
    assert np.all(it == v["max_iter"])
    assert np.array_equal(it, _unflagged("NUC201X")[0])
    assert counts[0] + counts[2] == v["max_iter"] * W * H
    _, dbl = XB.samples_x_bla(v, W, H, orbit=_orbit("NUC201X"), double_radius=True)
    print("NUC201X trips", counts[0] + counts[1], "with a double radius", dbl[0] + dbl[1])
    assert 10 * (counts[0] + counts[1]) < dbl[0] + dbl[1]
    emin = int(_orbit("NUC201X")[1][1:].min())
    assert emin < -1074                                              # below every double: why the radius is extended


@pytest.mark.parametrize("name", ["PX400A", "PX400B", "NUC201X"])
def test_table_shape_and_properties(name):
    v = XB.VIEWS[name]
    mant, exp2 = _orbit(name)
    N = len(exp2) - 1
    tab = XB.view_table(v, W, H, (mant, exp2))
    assert len(tab) == (N - 1).bit_length() - 1
    assert sum(len(T["rv"]) for T in tab) == (N - 1) - bin(N - 1).count("1")
    r, mb, ex = XB.table_arrays(tab)
    assert r.shape == (len(mb), 2) and mb.shape[1] == XB.ENTRY_DOUBLES and ex.shape == (len(mb), 2)
    assert r.itemsize * 2 + mb.itemsize * 12 + ex.itemsize * 2 == 112          # bytes per entry
    s = XB.single_steps_x(mant, exp2, v["p"], v["r"])
    as_float = lambda rv, re: np.where(rv == 0.0, -np.inf, np.log2(np.where(rv == 0.0, 1.0, rv)) + re)
    # no radius above 2^-54 (4 + |p|), the single steps' included
    cap = np.log2(4.0 + abs(v["p"])) - 54
    assert np.all(as_float(s["rv"], s["re"]) <= cap)
    prev_v, prev_e = s["rv"], s["re"]
    for k, T in enumerate(tab, 1):
        n = len(T["rv"])
        assert n == (N - 1) >> k
        assert np.all((T["rv"] == 0.0) | ((T["rv"] >= 0.5) & (T["rv"] < 1.0)))
        assert np.array_equal(T["rv"], T["rv"].astype(np.float32).astype(np.float64))       # 24 bits
        xv, xe = prev_v[0:2 * n:2], prev_e[0:2 * n:2]
        # monotone in k: an entry's radius is at most its first half's (the stored one is cut toward zero)
        assert np.all((T["re"] < xe) | ((T["re"] == xe) & (T["rv"] <= xv)))
        assert np.all(as_float(T["rv"], T["re"]) <= cap)
        for q in XB.ELEMS:                                            # mantissas normalised on the largest
            assert np.all(np.abs(T[q][0]) < 1.0) and np.all(np.abs(T[q][1]) < 1.0)
        if v["r"] == 0.0:
            for q in ("m12", "m22"):
                assert np.all(T[q][0] == 0.0) and np.all(T[q][1] == 0.0)
        prev_v, prev_e = T["rv"], T["re"]
    assert any(np.any(T["rv"] > 0.0) for T in tab)


def test_short_orbits_have_no_table():
    for max_iter in (1, 2):
        v = dict(PX.PX400A, max_iter=max_iter)
        orb = PX.orbit_of(v)
        assert XB.view_table(v, W, H, orb) == []
        (planes,), counts = XB.samples_x_bla(v, W, H, orbit=orb)
        plain = PX.samples_x(v, W, H, orbit=orb)[0]
        assert counts[1] == 0 and np.array_equal(planes[0], plain[0])
        for a, b in zip(planes, plain):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
