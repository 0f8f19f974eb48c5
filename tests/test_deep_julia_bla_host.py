"""BLA for deep Julia views (FR_FLAG_DEEP_JULIA_BLA, FR_FLAG_DEEPX_JULIA_BLA), everything that needs no GPU: the ABI, the
validation matrix of every deep validator against the two flags, the Python wrappers, the properties of both restated tables
(tests/deep_julia_bla_ref.py), and what the restated stepping gives against the unflagged restatement and the exact iteration."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import deep_julia_bla_ref as JB
import deep_julia_ref as J
import deepx_ref as X
from deepx_bla_ref import E_LIM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = JB.BW, JB.BH

# The iter values on which the restated flagged stepping equals the restated unflagged one, 128 x 96, aa 1 ("-x": through the
# extended restatements): measured here and asserted equal below, so that a change of either restatement shows.
# tests/test_deep_julia_bla_gpu.py takes its bars from these figures.
EQUAL_TO_UNFLAGGED = {"RABBIT30": 12288, "DENDRITE100": 12288, "PRECRIT60": 12288, "DENDRITE400-x": 12288, "PRECRIT60-x": 12288}
# The restated counts [single steps, BLA steps, updates skipped] and the BLA steps on (Q, P) of those frames
COUNTS = {
    "RABBIT30": ([5040999, 122051, 7050768], (71551, 50500)),
    "DENDRITE100": ([1456773, 42103, 7287094], (0, 42103)),
    "PRECRIT60": ([590644, 102997, 3204504], (35699, 67298)),
    "DENDRITE400-x": ([1459048, 62641, 33266902], (0, 62641)),       # 22.8 updates skipped per single step
    "PRECRIT60-x": ([590644, 102997, 3204504], (35699, 67298)),
}
# The flagged restatement's agreement with the exact fixed-point iteration on deep_julia_ref's 256 random samples (128 x 96;
# DENDRITE400: the 48 x 36 frame of exact_samples_x).  The largest exact class is 0.19 of the samples on both; RABBIT30's is
# 0.73, above the 0.60 of the class-collapse guard, so it is not among these views.
EXACT_AGREEMENT = {"DENDRITE100": 256, "DENDRITE400": 256}


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_header_macros_flags_and_symbols(fr, tmp_path):
    K = fr._capi
    assert fr.FR_FLAG_DEEP_JULIA_BLA == 0x20 == K.FR_FLAG_DEEP_JULIA_BLA
    assert fr.FR_FLAG_DEEPX_JULIA_BLA == 0x40 == K.FR_FLAG_DEEPX_JULIA_BLA
    assert "FR_FLAG_DEEP_JULIA_BLA" in fr.__all__ and "FR_FLAG_DEEPX_JULIA_BLA" in fr.__all__
    for name in ("fr_ctx_last_deep_julia_steps", "fr_ctx_last_deepx_julia_steps", "fr_deep_julia_bla_table",
                 "fr_deepx_julia_bla_table"):
        assert name in K.SIGNATURES and getattr(fr.lib(), name)
    assert "fr_deep_bla_builds" in K.INTERNAL_SIGNATURES and fr.lib().fr_deep_bla_builds
    assert callable(fr.Renderer.last_deep_julia_steps) and callable(fr.Renderer.last_deepx_julia_steps)
    hdr = open(os.path.join(ROOT, "include", "fractalrenderer_amd.h")).read()
    assert "Out of scope: BLA for Julia" not in hdr
    assert "There is no BLA for Julia views" not in fr.Renderer.render_deep_julia.__doc__
    gcc = shutil.which("gcc")
    if gcc:
        src = tmp_path / "macros.c"
        src.write_text("#include \"fractalrenderer_amd.h\"\n"
                       "#if !defined(FR_HAS_DEEP_JULIA_BLA) || FR_HAS_DEEP_JULIA_BLA != 1\n#error FR_HAS_DEEP_JULIA_BLA\n#endif\n"
                       "#if !defined(FR_HAS_DEEPX_JULIA_BLA) || FR_HAS_DEEPX_JULIA_BLA != 1\n#error FR_HAS_DEEPX_JULIA_BLA\n#endif\n"
                       "#if FR_FLAG_DEEP_JULIA_BLA != 0x20u || FR_FLAG_DEEPX_JULIA_BLA != 0x40u\n#error flag values\n#endif\n"
                       "#if ((FR_FLAG_DEEP_JULIA_BLA | FR_FLAG_DEEPX_JULIA_BLA) & (FR_FLAG_POST_CHAIN | FR_FLAG_DEEP_BLA | "
                       "FR_FLAG_DEEPX_BLA | FR_FLAG_DEEP_SHIP_BLA | FR_FLAG_DEEPX_SHIP_BLA)) != 0\n#error flag bits overlap\n#endif\n"
                       "int (*a)(fr_ctx*, uint64_t[3]) = fr_ctx_last_deep_julia_steps;\n"
                       "int (*b)(fr_ctx*, uint64_t[3]) = fr_ctx_last_deepx_julia_steps;\n"
                       "int64_t (*c)(fr_ctx*, double*, double*, int64_t) = fr_deep_julia_bla_table;\n"
                       "int64_t (*d)(fr_ctx*, void*, double*, int32_t*, int64_t) = fr_deepx_julia_bla_table;\n")
        subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "macros.o")], check=True)


# ---- validation ------------------------------------------------------------------------------------------------------------
def test_validation_matrix(fr):
    """each Julia entry point accepts its own flag and no other BLA flag; every other deep validator refuses both"""
    L, K = fr.lib(), fr._capi
    U = K.FR_ERR_UNSUPPORTED
    f64 = fr.Precision.F64
    dj, xj = K.FR_FLAG_DEEP_JULIA_BLA, K.FR_FLAG_DEEPX_JULIA_BLA
    old = (K.FR_FLAG_DEEP_BLA, K.FR_FLAG_DEEPX_BLA, K.FR_FLAG_DEEP_SHIP_BLA, K.FR_FLAG_DEEPX_SHIP_BLA)
    dv = K.fr_deep_view(b"0.1", b"0.2", 0, 0)
    xv = K.fr_deepx_view(b"0.1", b"0.2", b"1e-400", 0, 0)

    def check(fn, view, ftype, flags, zoom=1e-30):
        p = fr.FractalState(zoom=zoom, max_iterations=64).to_params(ftype, f64, False)
        p.flags |= flags
        return fn(C.byref(p), C.byref(view), 8, 8)

    julia = fr.FractalType.JuliaSet
    for fn, view, own, other in ((L.fr_deep_julia_validate, dv, dj, xj), (L.fr_deepx_julia_validate, xv, xj, dj)):
        assert check(fn, view, julia, 0) == 0 and check(fn, view, julia, own) == 0
        assert check(fn, view, julia, own | K.FR_FLAG_POST_CHAIN) == 0
        assert check(fn, view, julia, other) == U and check(fn, view, julia, own | other) == U
        for f in old:
            assert check(fn, view, julia, f) == U and check(fn, view, julia, f | own) == U, f
        assert check(fn, view, fr.FractalType.Mandelbrot, own) == U     # the other rules of the path hold with the flag
    others = ((L.fr_deep_validate, dv, fr.FractalType.Mandelbrot, K.FR_FLAG_DEEP_BLA),
              (L.fr_deepx_validate, xv, fr.FractalType.Mandelbrot, K.FR_FLAG_DEEPX_BLA),
              (L.fr_deep_ship_validate, dv, fr.FractalType.BurningShip, K.FR_FLAG_DEEP_SHIP_BLA),
              (L.fr_deepx_ship_validate, xv, fr.FractalType.BurningShip, K.FR_FLAG_DEEPX_SHIP_BLA))
    for fn, view, ftype, own in others:
        assert check(fn, view, ftype, 0) == 0 and check(fn, view, ftype, own) == 0
        for f in (dj, xj, dj | xj):
            assert check(fn, view, ftype, f) == U and check(fn, view, ftype, f | own) == U, (fn, f)
    # the sequence creators check their parameters by the same rules, before they look at the context
    d = K.fr_deep_sequence_desc(b"-2", b"0", b"1e-310", b"2.5e-311", 5, 0, 0, 0)
    resolve = C.CDLL(K.LIB_PATH).fr_deepseq_resolve_formula        # fr_internal.h: what both creators call first
    resolve.restype = C.c_int
    resolve.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    walk = (C.c_double * 8)()                                      # room for a fr_deepseq_walk (44 bytes)
    for ship, ftype in ((0, fr.FractalType.Mandelbrot), (1, fr.FractalType.BurningShip)):
        p = fr.FractalState(max_iterations=64).to_params(ftype, f64, False)
        assert resolve(C.byref(p), C.byref(d), 8, 8, ship, walk) == 0
        for f in (dj, xj):
            p.flags = f
            assert resolve(C.byref(p), C.byref(d), 8, 8, ship, walk) == U, (ship, f)


def test_python_wrappers(fr):
    """bla=True picks the flag by the view; the step readers refuse a context without such a render"""
    seen = {}

    class Probe(fr.Renderer):
        def __init__(self):
            self._lib = fr.lib()

        def _render_call(self, fn_sync, fn_async, params, *a):
            seen["flags"] = params[0]._obj.flags
            seen["extended"] = fn_sync is self._lib.fr_render_deepx_julia

    r = Probe()
    st = fr.FractalState(zoom=1e-30, max_iterations=64)
    r.render_deep_julia(st, 8, 8, fr.DeepView("0.1", "0.2"), bla=True)
    assert seen == {"flags": fr.FR_FLAG_DEEP_JULIA_BLA, "extended": False}
    r.render_deep_julia(st, 8, 8, fr.DeepView("0.1", "0.2", zoom="1e-400"), bla=True, post_chain=True)
    assert seen == {"flags": fr.FR_FLAG_DEEPX_JULIA_BLA | fr._capi.FR_FLAG_POST_CHAIN, "extended": True}
    r.render_deep_julia(st, 8, 8, fr.DeepView("0.1", "0.2", zoom="1e-400"))
    assert seen == {"flags": 0, "extended": True}
    for fn in (fr.lib().fr_ctx_last_deep_julia_steps, fr.lib().fr_ctx_last_deepx_julia_steps):
        assert fn(None, (C.c_uint64 * 3)()) == fr._capi.FR_ERR_INVALID_ARG
    assert fr.lib().fr_deep_julia_bla_table(None, None, None, 0) == fr._capi.FR_ERR_INVALID_ARG
    assert fr.lib().fr_deepx_julia_bla_table(None, None, None, None, 0) == fr._capi.FR_ERR_INVALID_ARG


# ---- the restated tables ---------------------------------------------------------------------------------------------------
def _check_levels(tab, N, r_of):
    assert len(tab) == ((N - 1).bit_length() - 1 if N > 1 else 0)
    assert sum(len(r_of(T)[0]) for T in tab) == JB.entries(N)
    for k, T in enumerate(tab, 1):
        assert len(r_of(T)[0]) == (N - 1) >> k


@pytest.mark.parametrize("name", ["RABBIT30", "DENDRITE100", "PRECRIT60", "BASILICA30"])
def test_table_properties(name):
    P, Q = JB.orbits(name)
    tq, tp = JB.bla_tables(P, Q)
    for orbit, tab in ((Q, tq), (P, tp)):
        N = len(orbit) - 1
        _check_levels(tab, N, lambda T: (T["r"],))
        prev = dict(r=JB.EPS * np.sqrt(orbit[1:N, 0] ** 2 + orbit[1:N, 1] ** 2))
        zero = (orbit[1:N, 0] == 0.0) & (orbit[1:N, 1] == 0.0)      # single steps at a Z_m = 0
        for k, T in enumerate(tab, 1):
            cnt = len(T["r"])
            assert (T["r"] <= prev["r"][0:2 * cnt:2]).all(), k        # monotone in k
            assert (T["r"] >= 0.0).all()
            assert (T["r"][~(np.isfinite(T["ax"]) & np.isfinite(T["ay"]))] == 0.0).all()   # A past a double: no radius
            zero = zero[0:2 * cnt:2] | zero[1:2 * cnt:2]              # the entry covers a zero
            assert (T["r"][zero] == 0.0).all(), k
            prev = T
    if name == "BASILICA30":                                        # Q = 0, -1, 0, -1, ...: every entry covers a zero
        assert np.array_equal(Q[:6], [[0, 0], [-1, 0], [0, 0], [-1, 0], [0, 0], [-1, 0]])
        assert len(tq) == 8 and all((T["r"] == 0.0).all() for T in tq)
        assert any((T["r"] > 0.0).any() for T in tp)
    else:
        assert all((T["r"] > 0.0).any() for T in tq[:6]) and all((T["r"] > 0.0).any() for T in tp[:6])


def _le(v, e, w, f):
    """(v, e) <= (w, f) on normalised extended reals"""
    return (e < f) | ((e == f) & (v <= w))


@pytest.mark.parametrize("name", ["DENDRITE400", "PRECRIT60", "BASILICA30"])
def test_extended_table_properties(name):
    Px, Qx = JB.orbits_x(name)
    tq, tp = JB.bla_tables_x(Px, Qx)
    for (mant, exp2), tab in ((Qx, tq), (Px, tp)):
        N = len(exp2) - 1
        _check_levels(tab, N, lambda T: (T["rv"],))
        nx, ny, ne = X._norm(mant[1:N, 0], mant[1:N, 1], exp2[1:N].astype(np.int64))
        zv, ze = JB.XB._norm1(np.sqrt(nx * nx + ny * ny), ne)
        prev = dict(rv=zv, re=np.where(zv == 0.0, X.X_ZERO, ze - 53))
        zero = zv == 0.0
        for k, T in enumerate(tab, 1):
            cnt = len(T["rv"])
            assert _le(T["rv"], T["re"], prev["rv"][0:2 * cnt:2], prev["re"][0:2 * cnt:2]).all(), k
            assert np.array_equal(T["rv"], T["rv"].astype(np.float32).astype(np.float64))   # a stored radius is a float
            assert (T["re"][T["rv"] == 0.0] == X.X_ZERO).all()
            big = np.maximum(np.abs(T["ax"]), np.abs(T["ay"]))
            assert ((big >= 0.5) & (big < 1.0) | (big == 0.0)).all()
            assert (np.abs(T["ea"][big > 0.0]) <= E_LIM).all() and (T["ea"][big == 0.0] == X.X_ZERO).all()
            zero = zero[0:2 * cnt:2] | zero[1:2 * cnt:2]
            assert (T["rv"][zero] == 0.0).all(), k
            prev = T
    if name == "BASILICA30":
        assert all((T["rv"] == 0.0).all() for T in tq) and any((T["rv"] > 0.0).any() for T in tp)


def test_no_table_for_short_orbits_and_c_zero():
    for N in (1, 2):
        orbit = np.array([[0.0, 0.0]] + [[0.3, 0.4]] * N)
        assert JB.bla_table(orbit) == [] and JB.entries(N) == 0
        assert JB.bla_table_x(orbit.copy(), np.array([X.X_ZERO] + [0] * N, np.int32)) == []
    assert [JB.entries(N) for N in (3, 4, 5, 9, 10, 17, 1000)] == [1, 1, 3, 7, 7, 15, 991]   # sum over k of (N - 1) >> k
    # c = 0: Q is zero throughout, P falls to zero; a table is there and every radius over a zero is 0
    v = dict(name="c0", c=(0.0, 0.0), cx="0.5", cy="0.25", zoom=1e-30, zoom_s="1e-30", max_iter=300, F=256)
    P, Q = J.reference_orbits(v)
    assert (Q == 0.0).all() and len(Q) == 301
    tq, tp = JB.bla_tables(P, Q)
    assert len(tq) == 8 and all((T["r"] == 0.0).all() for T in tq)
    assert (tp[0]["r"][:2] > 0.0).all() and (tp[-1]["r"] == 0.0).all()
    tqx, _ = JB.bla_tables_x(*J.reference_orbits_x(v))
    assert all((T["rv"] == 0.0).all() and (T["re"] == X.X_ZERO).all() for T in tqx)


def test_void_entries_appear_where_an_exponent_leaves_the_range():
    """No view of the suite reaches the void rule, so it is pinned on a synthetic orbit whose points sit at 2^(2^21): from
    level 6 on A's exponent, about 2^k (2^21 + 1), leaves [-2^27, 2^27], and the zeroed entries keep every level above void."""
    n = 1 + (1 << 8) + 1
    mant = np.tile(np.array([[0.75, -0.625]]), (n, 1))
    mant[0] = 0.0
    exp2 = np.full(n, 1 << 21, np.int32)
    exp2[0] = X.X_ZERO
    tab = JB.bla_table_x(mant, exp2)
    assert len(tab) == 8
    for k, T in enumerate(tab, 1):
        void = (1 << 21) * (1 << k) + (1 << k) > E_LIM
        assert ((T["ea"] == X.X_ZERO) == void).all(), k
        if void:
            assert (T["rv"] == 0.0).all() and (T["re"] == X.X_ZERO).all() and (T["ax"] == 0.0).all() and (T["ay"] == 0.0).all()
    assert any((T["ea"] == X.X_ZERO).all() for T in tab) and not (tab[0]["ea"] == X.X_ZERO).any()


# ---- the restated stepping -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(EQUAL_TO_UNFLAGGED))
def test_restated_stepping_against_the_unflagged_restatement(case):
    extended = case.endswith("-x")
    name = case[:-2] if extended else case
    v = JB.view(name)
    samples, counts, stats = (JB.restated_x_bla if extended else JB.restated_bla)(name)
    it, it0 = samples[0][0], (JB.unflagged_x if extended else JB.unflagged)(name)
    equal = int((it == it0).sum())
    print(case, "counts", counts, stats, "iter equal to the unflagged restatement", equal, "of", it.size,
          "skipped per single step", counts[2] / counts[0])
    assert equal == EQUAL_TO_UNFLAGGED[case]
    assert (list(counts), (stats["bla_q"], stats["bla_p"])) == COUNTS[case]
    # the counts are consistent: every update is a single step or skipped
    assert counts[0] + counts[2] == J.lane_updates(it, v["max_iter"])
    assert stats["bla_q"] + stats["bla_p"] == counts[1] > 0
    if name == "PRECRIT60":
        assert stats["bla_q"] > 0                                   # 35699: the view exists for the steps on Q
    if name == "DENDRITE400":
        assert counts[2] > counts[0]                                # 33266902 against 1459048: 22.8 to 1


@pytest.mark.parametrize("name", list(EXACT_AGREEMENT))
def test_agreement_with_the_exact_iteration(name):
    extended = name == "DENDRITE400"
    w, h = (J.XW, J.XH) if extended else (W, H)
    ex = J.exact_samples_x(name) if extended else J.exact_samples(name, w, h)
    ys, xs = J.random_pixels(w, h)
    it = (JB.restated_x_bla if extended else JB.restated_bla)(name, 1, w, h)[0][0][0]
    it0 = (JB.unflagged_x if extended else JB.unflagged)(name, w, h)
    largest = np.unique(ex, return_counts=True)[1].max() / len(ex)
    print(name, "largest exact class", largest, "agreement", int((it[ys, xs] == ex).sum()), "unflagged", int((it0[ys, xs] == ex).sum()))
    assert largest <= 0.60                                          # a collapsed frame cannot agree by chance
    assert int((it0[ys, xs] == ex).sum()) == 256
    assert int((it[ys, xs] == ex).sum()) == EXACT_AGREEMENT[name]
