"""BLA for extended views (FR_FLAG_DEEPX_BLA), no GPU: the ABI additions, the validation, and the numpy restatement
(tests/deepx_bla_ref.py) against the direct fixed-point iteration (tests/golden/deepx_exact.npz, deepx_ref.exact_iter_x).

The agreement bar is the project's: at least 0.99 of the golden samples equal the exact iteration, and no single exact
count holds more than 0.60 of them (a collapsed frame cannot agree by chance).  Measured with this restatement: 1.0 on
T130, T320 and D (256 samples each)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import deepx_bla_ref as XB
import deepx_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 256, 192
V = X.views()
D_ROWS = list(range(90, 102))


def test_header_macros_flag_and_symbols(fr, tmp_path):
    text = open(os.path.join(ROOT, "include", "fractalrenderer_amd.h")).read()
    assert re.search(r"#define\s+FR_FLAG_DEEPX_BLA\s+0x4u", text) and re.search(r"#define\s+FR_HAS_DEEPX_BLA\s+1\b", text)
    assert re.search(r"#define\s+FR_FLAG_DEEP_BLA\s+0x2u", text)
    assert "Out of scope: BLA for extended views" not in text
    assert "fr_deepx_bla_table" in open(os.path.join(ROOT, "fractalrenderer_amd", "csrc", "fr_internal.h")).read()
    assert fr.FR_FLAG_DEEPX_BLA == fr._capi.FR_FLAG_DEEPX_BLA == 0x4 and fr.FR_FLAG_DEEP_BLA == 0x2
    assert "fr_ctx_last_deepx_steps" in fr._capi.SIGNATURES and fr.lib().fr_ctx_last_deepx_steps
    assert "fr_deepx_bla_table" in fr._capi.INTERNAL_SIGNATURES and fr.lib().fr_deepx_bla_table
    assert callable(fr.Renderer.last_deepx_steps)
    assert fr.lib().fr_ctx_last_deepx_steps(None, (C.c_uint64 * 3)()) == fr._capi.FR_ERR_INVALID_ARG
    gcc = shutil.which("gcc")
    if gcc:
        src = tmp_path / "macros.c"
        src.write_text("#include <stdio.h>\n#include \"fractalrenderer_amd.h\"\n"
                       "#if !defined(FR_HAS_DEEPX_BLA) || FR_HAS_DEEPX_BLA != 1\n#error FR_HAS_DEEPX_BLA\n#endif\n"
                       "int main(void) { int (*f)(fr_ctx*, uint64_t*) = fr_ctx_last_deepx_steps; (void)f;\n"
                       "printf(\"%u %u\\n\", FR_FLAG_DEEPX_BLA, FR_FLAG_DEEP_BLA); return 0; }\n")
        subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "macros.o")], check=True)


def test_validate_accepts_the_new_flag_and_still_refuses_the_fp64_one(fr):
    L = fr.lib()
    U = fr._capi.FR_ERR_UNSUPPORTED
    v = V["D"]
    cv = fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"]).to_cx()

    def validate(flags):
        p = fr.FractalState(max_iterations=64).to_params(fr.FractalType.Mandelbrot, fr.Precision.F64, False)
        p.flags |= flags
        return L.fr_deepx_validate(C.byref(p), C.byref(cv), 8, 8)

    assert validate(0) == 0 and validate(fr.FR_FLAG_DEEPX_BLA) == 0
    assert validate(fr.FR_FLAG_DEEPX_BLA | fr._capi.FR_FLAG_POST_CHAIN) == 0
    assert validate(fr.FR_FLAG_DEEP_BLA) == U and validate(fr.FR_FLAG_DEEP_BLA | fr.FR_FLAG_DEEPX_BLA) == U


def test_python_keyword_needs_a_zoom_string(fr):
    """checked before anything touches a device: Renderer.render_deep is called unbound on an object without a context"""
    with pytest.raises(ValueError):
        fr.Renderer.render_deep(object(), fr.FractalState(), 8, 8, fr.DeepView("0", "0"), xbla=True)
    with pytest.raises(ValueError):
        fr.Renderer.render_deep(object(), fr.FractalState(), 8, 8, None, xbla=True)


def _check(name, it_at_golden):
    ex = X.exact_golden()[name]
    share = float(np.unique(ex, return_counts=True)[1].max()) / len(ex)
    agree = float((it_at_golden == ex).mean())
    print(name, "largest share of one exact count", share, "agreement with the exact iteration", agree)
    assert share <= 0.60
    assert agree >= 0.99


@pytest.mark.parametrize("name", ["T130", "T320"])
def test_restatement_agrees_with_the_exact_iteration_on_whole_frames(name):
    g = X.exact_golden()
    v = V[name]
    samples, counts = XB.restate_x_bla(v, W, H)
    it = samples[0][0]
    print(name, "counts", counts)
    _check(name, it[g["ys"], g["xs"]])
    assert counts[1] > 0 and counts[2] > counts[0]
    assert counts[0] + counts[2] == int(np.where(it < v["max_iter"], it + 1, v["max_iter"]).sum())
    for k in (0, 97, 255):                                          # the fixture is what exact_iter_x gives
        assert X.exact_iter_x(v, int(g["xs"][k]), int(g["ys"][k]), W, H) == g[name][k], k


def test_restatement_on_view_d():
    """the golden samples of D one by one, and a band of rows for the counts: BLA steps are taken, and they skip more
    updates than single steps are left"""
    g = X.exact_golden()
    v = V["D"]
    orbit = X.orbit_of(v)
    table = XB.table_of(v, W, H, orbit)
    assert len(table) == 11 and all((T["rv"] > 0).all() for T in table)
    zm, ze = X.zoom_pair(v["zoom"])
    dc = X.sample_dc_x(W, H, zm, ze, 1, 0, rows=g["ys"])
    sel = np.arange(len(g["ys"])) * W + g["xs"]
    it, _, c = XB.perturb_x_bla(orbit[0], orbit[1], tuple(a[sel] for a in dc), v["max_iter"], table)
    _check("D", it)
    assert c[1] > 0 and c[2] > c[0]
    samples, counts = XB.restate_x_bla(v, W, H, rows=D_ROWS, orbit=orbit, table=table)
    plain = X.restate_x(v, W, H, rows=D_ROWS, orbit=orbit)
    print("D rows", D_ROWS[0], "..", D_ROWS[-1], "counts", counts, "iter equal to the restatement without BLA",
          float((samples[0][0] == plain[0][0]).mean()))
    assert counts[1] > 0 and counts[2] > counts[0]
    assert (samples[0][0] == plain[0][0]).mean() >= 0.999


def test_table_radii_are_floats_and_shrink_with_the_level():
    """a stored radius keeps 24 bits, and r of an entry never exceeds r of its first half"""
    v = V["T300"]
    table = XB.table_of(v, W, H, X.orbit_of(v))
    for k, T in enumerate(table):
        assert np.array_equal(T["rv"], T["rv"].astype(np.float32).astype(np.float64))
        assert ((T["rv"] == 0) | ((T["rv"] >= 0.5) & (T["rv"] < 1.0))).all()
        assert (np.abs(T["ea"]) <= XB.E_LIM).all() and (np.abs(T["eb"]) <= XB.E_LIM).all()
        if k:
            P = table[k - 1]
            n = len(T["rv"])
            px, pe = P["rv"][0:2 * n:2], P["re"][0:2 * n:2]
            assert ((T["re"] < pe) | ((T["re"] == pe) & (T["rv"] <= px))).all()


def test_a_zero_orbit_gives_a_void_table_and_no_bla_step():
    v = dict(cx="0", cy="0", zoom="1e-320", max_iter=200)
    orbit = X.orbit_of(v)
    table = XB.table_of(v, 64, 48, orbit)
    assert table and all((T["rv"] == 0).all() and (T["re"] == X.X_ZERO).all() for T in table)
    samples, counts = XB.restate_x_bla(v, 64, 48, orbit=orbit, table=table)
    plain = X.restate_x(v, 64, 48, orbit=orbit)
    assert counts[1:] == [0, 0]
    assert np.array_equal(samples[0][0], plain[0][0]) and np.array_equal(samples[0][1].view(np.uint64), plain[0][1].view(np.uint64))
