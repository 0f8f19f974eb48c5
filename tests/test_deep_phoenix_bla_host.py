"""Deep Phoenix views with bilinear approximation (FR_FLAG_DEEP_PHOENIX_BLA): the parts that need no GPU -- the ABI, the
validation, the Python wrapper, and what the restatement (tests/deep_phoenix_bla_ref.py) skips, where it stands against the
unflagged restatement and the exact fixed-point iteration, and the shape of its table."""
import ctypes as C
import functools
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import deep_phoenix_bla_ref as PB
import deep_phoenix_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = (24, 18)
W, H = 48, 36
DEEP = ("PA30", "PB30", "PA", "PB")
BUDGETS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33)

# [plain steps, BLA steps, updates skipped] of the restatement at 48 x 36, aa 1, and the share of the updates it skips: taken
# from the restatement (never from a device), so that a change of the rule or of its restatement shows
PINNED = {
    "PA30": ((313108, 7546, 185488), 0.3720),
    "PB30": ((439231, 10803, 332190), 0.4306),
    "PA": ((282735, 11547, 1098772), 0.7953),
    "PB": ((557115, 7254, 1808644), 0.7645),
}


@functools.lru_cache(maxsize=None)
def _orbit(name):
    return D.view_orbit(D.VIEWS[name])


@functools.lru_cache(maxsize=None)
def _flagged(name, w, h):
    """computed once per (view, size), shared, never changed"""
    (planes,), counts = PB.samples_bla(D.VIEWS[name], w, h, orbit=_orbit(name))
    return planes, tuple(counts)


@functools.lru_cache(maxsize=None)
def _unflagged(name, w, h):
    (planes,), _ = D.samples(D.VIEWS[name], w, h, orbit=_orbit(name))
    return planes


def _updates(it, max_iter):
    return int(np.where(it < max_iter, it.astype(np.int64) + 1, max_iter).sum())


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_flag_counts_and_table_are_in_the_header_and_capi(fr, tmp_path):
    K = fr._capi
    hdr = open(os.path.join(ROOT, "include", "fractalrenderer_amd.h")).read()
    assert re.search(r"#define FR_FLAG_DEEP_PHOENIX_BLA\s+0x80u", hdr)
    assert re.search(r"#define FR_HAS_DEEP_PHOENIX_BLA 1", hdr)
    assert re.search(r"int fr_ctx_last_deep_phoenix_steps\(fr_ctx\* ctx, uint64_t out\[3\]\);", hdr)
    assert "Out of scope: BLA, distance estimates" not in hdr
    internal = open(os.path.join(ROOT, "fractalrenderer_amd", "csrc", "fr_internal.h")).read()
    assert re.search(r"int64_t fr_deep_phoenix_bla_table\(fr_ctx\* ctx, double\* r, double\* mb, int64_t n\);", internal)
    assert K.FR_FLAG_DEEP_PHOENIX_BLA == 0x80 == fr.FR_FLAG_DEEP_PHOENIX_BLA
    assert "FR_FLAG_DEEP_PHOENIX_BLA" in fr.__all__
    assert "fr_ctx_last_deep_phoenix_steps" in K.SIGNATURES
    assert "fr_deep_phoenix_bla_table" in K.INTERNAL_SIGNATURES
    assert hasattr(fr.lib(), "fr_ctx_last_deep_phoenix_steps") and hasattr(fr.lib(), "fr_deep_phoenix_bla_table")
    assert inspect.signature(fr.Renderer.render_deep_phoenix).parameters["bla"].default is False
    assert callable(fr.Renderer.last_deep_phoenix_steps)
    flags = (K.FR_FLAG_POST_CHAIN, fr.FR_FLAG_DEEP_BLA, fr.FR_FLAG_DEEPX_BLA, fr.FR_FLAG_DEEP_SHIP_BLA, fr.FR_FLAG_DEEPX_SHIP_BLA,
             fr.FR_FLAG_DEEP_JULIA_BLA, fr.FR_FLAG_DEEPX_JULIA_BLA, fr.FR_FLAG_DEEP_PHOENIX_BLA)
    assert sorted(flags) == [1, 2, 4, 8, 16, 32, 64, 128]
    assert fr.lib().fr_ctx_last_deep_phoenix_steps(None, (C.c_uint64 * 3)()) == K.FR_ERR_INVALID_ARG
    assert fr.lib().fr_deep_phoenix_bla_table(None, None, None, 0) == K.FR_ERR_INVALID_ARG
    gcc = shutil.which("gcc")
    if gcc:
        src = tmp_path / "macros.c"
        src.write_text("#include \"fractalrenderer_amd.h\"\n"
                       "#if !defined(FR_HAS_DEEP_PHOENIX_BLA) || FR_HAS_DEEP_PHOENIX_BLA != 1\n#error FR_HAS_DEEP_PHOENIX_BLA\n#endif\n"
                       "#if FR_FLAG_DEEP_PHOENIX_BLA != 0x80u\n#error flag value\n#endif\n"
                       "#if (FR_FLAG_DEEP_PHOENIX_BLA & (FR_FLAG_POST_CHAIN | FR_FLAG_DEEP_BLA | FR_FLAG_DEEPX_BLA | "
                       "FR_FLAG_DEEP_SHIP_BLA | FR_FLAG_DEEPX_SHIP_BLA | FR_FLAG_DEEP_JULIA_BLA | FR_FLAG_DEEPX_JULIA_BLA)) != 0\n"
                       "#error flag bits overlap\n#endif\n"
                       "int (*a)(fr_ctx*, uint64_t[3]) = fr_ctx_last_deep_phoenix_steps;\n")
        subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "macros.o")], check=True)


def test_the_wrapper_sets_exactly_that_flag(fr):
    seen = {}

    class Probe(fr.Renderer):
        def __init__(self):
            self._lib = fr.lib()

        def _render_call(self, fn_sync, fn_async, params, *a):
            seen["flags"] = params[0]._obj.flags
            seen["entry"] = fn_sync is self._lib.fr_render_deep_phoenix and fn_async is self._lib.fr_render_deep_phoenix_async

    r = Probe()
    st = fr.FractalState(zoom=1e-30, max_iterations=64)
    view = fr.DeepView("0.1", "0.2")
    r.render_deep_phoenix(st, 8, 8, view, fr.PhoenixParams(), bla=True)
    assert seen == {"flags": fr.FR_FLAG_DEEP_PHOENIX_BLA, "entry": True}
    r.render_deep_phoenix(st, 8, 8, view, fr.PhoenixParams(), bla=True, post_chain=True)
    assert seen == {"flags": fr.FR_FLAG_DEEP_PHOENIX_BLA | fr._capi.FR_FLAG_POST_CHAIN, "entry": True}
    r.render_deep_phoenix(st, 8, 8, view, fr.PhoenixParams())
    assert seen == {"flags": 0, "entry": True}
    assert "bla" not in inspect.signature(fr.Renderer.render_deepx_phoenix).parameters


# ---- validation ------------------------------------------------------------------------------------------------------------
def test_validators(fr):
    """fr_deep_phoenix_validate accepts its flag and keeps refusing the six older ones, alone or next to it;
    fr_deepx_phoenix_validate refuses all seven"""
    L, K = fr.lib(), fr._capi
    U = K.FR_ERR_UNSUPPORTED
    own = K.FR_FLAG_DEEP_PHOENIX_BLA
    old = (K.FR_FLAG_DEEP_BLA, K.FR_FLAG_DEEPX_BLA, K.FR_FLAG_DEEP_SHIP_BLA, K.FR_FLAG_DEEPX_SHIP_BLA, K.FR_FLAG_DEEP_JULIA_BLA,
           K.FR_FLAG_DEEPX_JULIA_BLA)
    ph = fr.PhoenixParams().to_c()
    dv = K.fr_deep_view(b"0.1", b"0.2", 0, 0)
    xv = K.fr_deepx_view(b"0.1", b"0.2", b"1e-400", 0, 0)

    def check(fn, view, flags, ftype=fr.FractalType.Phoenix):
        p = fr.FractalState(zoom=1e-30, max_iterations=64).to_params(ftype, fr.Precision.F64, False)
        p.flags |= flags
        st = fn(C.byref(p), C.byref(ph), C.byref(view), 8, 8)
        return st, (L.fr_last_error() or b"").decode() if st else ""

    deep, deepx = L.fr_deep_phoenix_validate, L.fr_deepx_phoenix_validate
    assert check(deep, dv, 0)[0] == 0 and check(deep, dv, own)[0] == 0 and check(deep, dv, own | K.FR_FLAG_POST_CHAIN)[0] == 0
    for f in old:
        for flags in (f, f | own):
            st, msg = check(deep, dv, flags)
            assert st == U and "BLA" in msg, (flags, msg)
    assert check(deep, dv, own, fr.FractalType.Mandelbrot)[0] == U        # the other rules of the path hold with the flag
    assert check(deepx, xv, 0)[0] == 0
    for flags in (own, own | K.FR_FLAG_POST_CHAIN) + old + tuple(f | own for f in old):
        st, msg = check(deepx, xv, flags)
        assert st == U and "BLA" in msg, (flags, msg)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DEEP)
def test_iter_equals_the_unflagged_restatement_and_the_exact_iteration(name):
    """24 x 18: on every pixel, and plain + skipped is the unflagged update count"""
    w, h = SMALL
    v = D.VIEWS[name]
    (it, _, _, _), counts = _flagged(name, w, h)
    pit = _unflagged(name, w, h)[0]
    assert np.array_equal(it, pit), int((it != pit).sum())
    assert np.array_equal(it, D.exact_frame(v, w, h))
    assert counts[1] > 0
    assert counts[0] + counts[2] == _updates(pit, v["max_iter"])


@pytest.mark.parametrize("name", DEEP)
def test_what_the_restatement_skips_is_pinned(name):
    """48 x 36, aa 1"""
    v = D.VIEWS[name]
    (it, _, _, _), counts = _flagged(name, W, H)
    want, share = PINNED[name]
    print(name, "N", len(_orbit(name)) - 1, "counts", counts)
    assert len(_orbit(name)) - 1 == D.ORBIT_N[name]
    assert counts == want
    assert np.array_equal(it, _unflagged(name, W, H)[0])
    updates = _updates(it, v["max_iter"])
    assert counts[0] + counts[2] == updates                          # every update is a plain step or skipped
    assert round(counts[2] / updates, 4) == share


@pytest.mark.parametrize("name", ["shallowA", "mini0", "miniR"])
def test_no_bla_step_where_dc_is_above_every_radius(name):
    v = D.VIEWS[name]
    planes, counts = _flagged(name, W, H)
    plain = _unflagged(name, W, H)
    assert counts[1] == 0 and counts[2] == 0
    assert counts[0] == _updates(plain[0], v["max_iter"])
    for a, b in zip(planes, plain):                                  # and the planes are the plain step's, bit for bit
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("name", ["PA30", "PA"])
def test_aa_2_and_short_budgets(name):
    w, h = SMALL
    v = D.VIEWS[name]
    smp, _ = PB.samples_bla(v, w, h, 2, orbit=_orbit(name))
    plain, _ = D.samples(v, w, h, 2, orbit=_orbit(name))
    assert len(smp) == 4
    for a, b in zip(smp, plain):
        assert np.array_equal(a[0], b[0])
    for max_iter in BUDGETS:
        vv = dict(v, max_iter=max_iter)
        orb = D.view_orbit(vv)
        (a,), counts = PB.samples_bla(vv, w, h, orbit=orb)
        (b,), _ = D.samples(vv, w, h, orbit=orb)
        assert np.array_equal(a[0], b[0]), max_iter
        assert counts[0] + counts[2] == _updates(b[0], max_iter), max_iter
        if len(orb) - 1 <= 2:
            assert PB.view_table(vv, w, h, orb) == [] and counts[1] == 0


def test_without_radius_it_is_the_plain_step():
    """eps = 0: every radius is 0, no BLA step is taken and the planes are deep_phoenix_ref.perturb's, bit for bit"""
    w, h = SMALL
    (planes,), counts = PB.samples_bla(D.PA, w, h, orbit=_orbit("PA"), eps=0.0)
    assert counts[1] == 0 and counts[2] == 0
    for a, b in zip(planes, _unflagged("PA", w, h)):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("name", ["PA30", "PA"])
def test_table_shape_and_monotone_radius(name):
    v = D.VIEWS[name]
    orb = _orbit(name)
    N = len(orb) - 1
    tab = PB.view_table(v, W, H, orb)
    assert len(tab) == (N - 1).bit_length() - 1
    assert sum(len(T["r"]) for T in tab) == (N - 1) - bin(N - 1).count("1")
    r, mb = PB.table_arrays(tab)
    assert r.shape == (len(mb),) and mb.shape[1] == PB.ENTRY_DOUBLES
    prev = PB.single_steps(orb, v["p"], v["r"])["r"]
    for k, T in enumerate(tab, 1):
        assert len(T["r"]) == (N - 1) >> k
        assert np.all(T["r"] >= 0.0) and np.all(T["r"] <= prev[0:2 * len(T["r"]):2])
        prev = T["r"]
    assert any(np.any(T["r"] > 0.0) for T in tab)
    # level 1 in closed form: M = [[a_y a_x + r, a_y r], [a_x, r]], B = (a_y + 1, 1)
    s = PB.single_steps(orb, v["p"], v["r"])
    T = tab[0]
    n = len(T["r"])
    rr = np.float64(np.float32(v["r"]))
    assert np.array_equal(T["m21"][0], s["m11"][0][0:2 * n:2]) and np.array_equal(T["m21"][1], s["m11"][1][0:2 * n:2])
    assert np.all(T["m22"][0] == rr) and np.all(T["m22"][1] == 0.0)
    assert np.all(T["b2"][0] == 1.0) and np.all(T["b2"][1] == 0.0)
    assert np.array_equal(T["b1"][0], s["m11"][0][1:2 * n:2] + 1.0)
