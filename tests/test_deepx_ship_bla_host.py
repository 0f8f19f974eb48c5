"""BLA for extended Burning Ship views (fr_render_deepx_ship with FR_FLAG_DEEPX_SHIP_BLA), everything that needs no GPU: the
ABI, the validation rules, the Python wrappers' argument checks, the properties of the restated table
(tests/deepx_ship_bla_ref.py) and what the restated stepping gives against the unflagged restatement."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import deepx_ref as X
import deepx_ship_bla_ref as XB
import deepx_ship_ref as SX
from deepx_bla_ref import E_LIM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = SX.views()
EPS_EXP = -53

# The share of iter values on which the restated flagged stepping equals the restated unflagged one, 128 x 96, aa 1: measured
# here and asserted equal below, so that a change of either restatement shows.  tests/test_deepx_ship_bla_gpu.py takes its
# bars from these figures.
EQUAL_TO_UNFLAGGED = {"S400": 12279, "S310": 12241}                   # of 12288


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_header_macro_flag_and_symbols(fr, tmp_path):
    assert fr.FR_FLAG_DEEPX_SHIP_BLA == 0x10 == fr._capi.FR_FLAG_DEEPX_SHIP_BLA
    assert "fr_ctx_last_deepx_ship_steps" in fr._capi.SIGNATURES and fr.lib().fr_ctx_last_deepx_ship_steps
    assert "fr_deepx_ship_bla_table" in fr._capi.INTERNAL_SIGNATURES and fr.lib().fr_deepx_ship_bla_table
    assert callable(fr.Renderer.last_deepx_ship_steps)
    gcc = shutil.which("gcc")
    if gcc:
        src = tmp_path / "macros.c"
        src.write_text("#include \"fractalrenderer_amd.h\"\n"
                       "#if !defined(FR_HAS_DEEPX_SHIP_BLA) || FR_HAS_DEEPX_SHIP_BLA != 1\n#error FR_HAS_DEEPX_SHIP_BLA\n#endif\n"
                       "#if FR_FLAG_DEEPX_SHIP_BLA != 0x10u\n#error FR_FLAG_DEEPX_SHIP_BLA\n#endif\n"
                       "#if (FR_FLAG_DEEPX_SHIP_BLA & (FR_FLAG_POST_CHAIN | FR_FLAG_DEEP_BLA | FR_FLAG_DEEPX_BLA | "
                       "FR_FLAG_DEEP_SHIP_BLA)) != 0\n#error flag bits overlap\n#endif\n"
                       "int (*a)(fr_ctx*, uint64_t[3]) = fr_ctx_last_deepx_ship_steps;\n")
        subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "macros.o")], check=True)


# ---- validation ------------------------------------------------------------------------------------------------------------
def test_validation_of_the_flags(fr):
    L, K = fr.lib(), fr._capi
    U = K.FR_ERR_UNSUPPORTED
    ship, f64 = fr.FractalType.BurningShip, fr.Precision.F64
    v = K.fr_deepx_view(b"-2", b"0", b"1e-400", 0, 0)

    def check(flags, ftype=ship):
        p = fr.FractalState(max_iterations=64).to_params(ftype, f64, False)
        p.flags |= flags
        return L.fr_deepx_ship_validate(C.byref(p), C.byref(v), 8, 8)

    new = K.FR_FLAG_DEEPX_SHIP_BLA
    old = (K.FR_FLAG_DEEP_BLA, K.FR_FLAG_DEEPX_BLA, K.FR_FLAG_DEEP_SHIP_BLA)
    assert check(0) == 0 and check(new) == 0 and check(new | K.FR_FLAG_POST_CHAIN) == 0
    for f in old:
        assert check(f) == U and check(f | new) == U, f
    assert check(old[0] | old[1] | old[2] | new) == U
    assert check(new, fr.FractalType.Mandelbrot) == U              # the other rules of the path hold with the flag
    # the sequence's descriptor check goes through the same rules
    d = K.fr_deep_sequence_desc(b"-2", b"0", b"1e-310", b"2.5e-311", 5, 0, 0, 0)
    h = C.c_void_p()
    p = fr.FractalState(max_iterations=64).to_params(ship, f64, False)
    p.flags |= new
    assert L.fr_deep_ship_sequence_create(None, C.byref(p), C.byref(d), 8, 8, C.byref(h)) == K.FR_ERR_INVALID_ARG   # ctx NULL


def test_python_wrappers_reject_what_the_issue_names(fr):
    seq = functools.partial(fr.DeepZoomSequence, None, fr.FractalState(), "-2", "0", "1e-310", "2.5e-311", 5, 8, 8)
    with pytest.raises(ValueError):
        seq(formula="ship", xbla=True)
    with pytest.raises(ValueError):
        seq(formula="ship", xbla=True, bla=True)
    with pytest.raises(ValueError):
        seq(bla=True)                                               # the Mandelbrot formula has xbla
    with pytest.raises(ValueError):
        seq(formula="mandelbrot", bla=True, xbla=True)
    with pytest.raises(ValueError):                                 # a view without a zoom string, flag or not
        fr.Renderer.render_deepx_ship(None, fr.FractalState(), 8, 8, fr.DeepView("-2", "0"), bla=True)


# ---- the restated table ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _orbit(name):
    return SX.orbit_of(V[name])


@functools.lru_cache(maxsize=None)
def _table(name, W, H):
    return XB.table_of(V[name], W, H, _orbit(name))


def _le(v, e, w, f):
    """(v, e) <= (w, f) on normalised extended reals"""
    return (e < f) | ((e == f) & (v <= w))


@pytest.mark.parametrize("name,W,H", [("S400", 128, 96), ("TIPY300", 48, 36)])
def test_table_properties(name, W, H):
    mant, exp2 = _orbit(name)
    N = len(exp2) - 1
    tab = _table(name, W, H)
    assert len(tab) == (N - 1).bit_length() - 1
    assert sum(len(T["rv"]) for T in tab) == (N - 1) - bin(N - 1).count("1")
    single = XB.single_steps_x(mant, exp2)
    # the single step: r <= eps |Z_m| and r no larger than either stored coordinate
    nx, ny, ne = X._norm(mant[1:N, 0], mant[1:N, 1], exp2[1:N].astype(np.int64))
    zv, ze = XB._norm1(np.sqrt(nx * nx + ny * ny), ne)
    assert _le(single["rv"], single["re"], zv, np.where(zv == 0.0, X.X_ZERO, ze + EPS_EXP)).all()
    for col in (0, 1):
        cv, ce = XB._norm1(np.abs(mant[1:N, col]), exp2[1:N].astype(np.int64))
        assert _le(single["rv"], single["re"], cv, ce).all()
    prev = single
    for k, T in enumerate(tab, 1):
        cnt = len(T["rv"])
        assert cnt == (N - 1) >> k
        # r is monotone in k: no entry's r exceeds that of its first half
        assert _le(T["rv"], T["re"], prev["rv"][0:2 * cnt:2], prev["re"][0:2 * cnt:2]).all(), k
        # a stored radius is a float
        assert np.array_equal(T["rv"], T["rv"].astype(np.float32).astype(np.float64))
        zero = T["rv"] == 0.0
        assert (T["re"][zero] == X.X_ZERO).all()
        # normalised matrices: the largest mantissa in [0.5, 1) unless the matrix is zero
        for els, e in ((XB.A_ELEMS, "ea"), (XB.B_ELEMS, "eb")):
            big = np.max([np.abs(T[q]) for q in els], axis=0)
            assert ((big >= 0.5) & (big < 1.0) | (big == 0.0)).all()
            assert (np.abs(T[e][big > 0.0]) <= E_LIM).all()
            assert (T[e][big == 0.0] == X.X_ZERO).all()
        # void entries zero all three fields
        void = (T["ea"] == X.X_ZERO) | (T["eb"] == X.X_ZERO)
        assert (T["rv"][void] == 0.0).all() and (T["ea"][void] == X.X_ZERO).all() and (T["eb"][void] == X.X_ZERO).all()
        for q in XB.ELEMS:
            assert (T[q][void] == 0.0).all()
        prev = T
    if name == "S400":                                            # every level, the top one included, has usable entries
        assert all((T["rv"] > 0.0).any() for T in tab)
        assert not any(((T["ea"] == X.X_ZERO) | (T["eb"] == X.X_ZERO)).any() for T in tab)
    else:                                                         # Y starts 2^-1000 below X: there the fold cap |Y| is the radius
        yv, ye = XB._norm1(np.abs(mant[1:N, 1]), exp2[1:N].astype(np.int64))
        capped = XB._less(yv, ye, zv, ze + EPS_EXP)
        assert capped[0] and single["re"][0] < -900 and 100 < capped.sum() < N - 1
        assert (single["rv"][capped] == yv[capped]).all() and (single["re"][capped] == ye[capped]).all()
        assert (single["rv"] > 0.0).all()


def test_void_entries_appear_where_an_exponent_leaves_the_range():
    """No view of the suite reaches the void rule (S310's and NUC546's zero top-level entries are zero by the radius rule
    alone), so it is pinned on a synthetic orbit whose points sit at 2^(2^21): from level 6 on A's exponent, about
    2^k (2^21 + 1), leaves [-2^27, 2^27], and the zeroed entries keep every level above them void."""
    n = 1 + (1 << 8) + 1
    mant = np.tile(np.array([[0.75, -0.625]]), (n, 1))
    mant[0] = 0.0
    exp2 = np.full(n, 1 << 21, np.int32)
    exp2[0] = X.X_ZERO
    tab = XB.bla_table_ship_x(mant, exp2, (0.5, -1300))
    assert len(tab) == 8
    for k, T in enumerate(tab, 1):
        void = (1 << 21) * (1 << k) + (1 << k) > E_LIM
        assert ((T["ea"] == X.X_ZERO) == void).all(), k
        if void:
            assert (T["rv"] == 0.0).all() and (T["re"] == X.X_ZERO).all() and (T["eb"] == X.X_ZERO).all()
            assert all((T[q] == 0.0).all() for q in XB.ELEMS)
    assert any((T["ea"] == X.X_ZERO).all() for T in tab) and not (tab[0]["ea"] == X.X_ZERO).any()


def test_a_coordinate_stored_as_zero_gives_no_radius():
    """TIP400: the centre is on the real axis, Y = 0 on the whole orbit -- r = 0 for every single step and every entry"""
    mant, exp2 = _orbit("TIP400")
    assert (mant[:, 1] == 0.0).all()
    single = XB.single_steps_x(mant, exp2)
    assert (single["rv"] == 0.0).all() and (single["re"] == X.X_ZERO).all()
    tab = _table("TIP400", 64, 48)
    assert len(tab) == 10 and all((T["rv"] == 0.0).all() and (T["re"] == X.X_ZERO).all() for T in tab)


def test_dcmax_is_the_ship_formula_on_the_zoom_pair():
    import deep_ship_bla_ref as SB
    for W, H, zoom in ((128, 96, "1e-400"), (203, 117, "3.7e-310"), (48, 36, "1e-1000"), (64, 48, "1e-20")):
        zm, ze = X.zoom_pair(zoom)
        v, e = XB.dcmax_ship_x(W, H, zm, ze)
        assert 0.5 <= v < 1.0
        assert v * 2.0 ** (e - ze) == SB.dcmax(W, H, zm)           # a power-of-two rescaling of the fp64 formula


# ---- the restated stepping -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S400", "S310"])
def test_restated_stepping_against_the_unflagged_restatement(name):
    v = V[name]
    W, H = 128, 96
    samples, counts = XB.restate_ship_x_bla(v, W, H, orbit=_orbit(name), table=_table(name, W, H))
    plain = SX.restate_ship_x(v, W, H, orbit=_orbit(name))
    it, it0 = samples[0][0], plain[0][0]
    equal = int((it == it0).sum())
    print(name, "counts", counts, "iter equal to the unflagged restatement", equal, "of", it.size,
          "largest |difference|", int(np.abs(it.astype(np.int64) - it0).max()))
    assert equal == EQUAL_TO_UNFLAGGED[name]
    # the counts are consistent: every update is a single step or skipped
    upd = int(np.where(it < v["max_iter"], it + 1, v["max_iter"]).sum())
    assert counts[0] + counts[2] == upd
    assert counts[1] > 0 and counts[2] > 10 * counts[0]            # more than nine tenths of the updates are skipped
    # against the direct fixed-point iteration on the recorded samples: 256 of 256 on both views, as the unflagged restatement
    g = SX.exact_golden()
    assert int((it[g["ys"], g["xs"]] == g[name]).sum()) == 256
