"""The extended deep kernels on lanes that fall back from the plain mode to the extended one, dozens of times each (views
RET130 and RET320 of tests/deepx_return_ref.py): fr_render_deepx plain and with FR_FLAG_DEEPX_BLA, fr_render_deepx_de in both
forms and fr_render_deepx_phoenix at p = r = 0 against the restatements and the exact iteration recorded in
tests/golden/deepx_return.npz, and against fr_render_deep, which has no extended mode, where it accepts the view.  24 x 18
frames, aa 1; one ragged frame with aa 2 and the post chain."""
import functools

import numpy as np
import pytest

import deep_phoenix_ref as D
import deep_ref as R
import deepx_de_ref as XD
import deepx_ref as X
import deepx_return_ref as RET
from test_deep_de_gpu import _check_de, _same_bytes
from test_deep_phoenix_gpu import NU_TOL as PX_NU_TOL
from test_deepx_de_gpu import _render_de
from test_deepx_gpu import _check_planes, _render_plain, _render_x
from test_deepx_phoenix_gpu import _render as _render_phoenix

pytestmark = pytest.mark.gpu

W, H = RET.SIZE
V = RET.views()
RAGGED = (31, 23)                  # no multiple of the 8 x 8 sub-tile either way


def _check_exact(name, it, phoenix=False):
    ys, xs = RET.exact_pixels(name)
    ex = RET.exact(name, phoenix)
    print(name, "pixels that differ from the exact iteration", int((it[ys, xs] != ex).sum()), "of", ex.size)
    assert np.array_equal(it[ys, xs], ex)


@pytest.mark.parametrize("name", RET.NAMES)
def test_planes_are_the_restatement_and_iter_the_exact_iteration(fr, renderer, oracle, name):
    got = _render_x(fr, renderer, V[name], w=W, h=H)
    st = RET.stats(name)
    print(name, st)
    assert st["to_ext"] >= 20 * W * H                                # the reason these views exist
    _check_planes(oracle, V[name], got, [(RET.golden(name, "iter"), RET.golden(name, "r2"))], 1, False)
    _check_exact(name, got[2])


def test_ret130_is_byte_for_byte_fr_render_deep(fr, renderer):
    """fr_render_deep never leaves fp64: an independent kernel.  The two CPU restatements differ on no pixel and in no bit of r2
    (test_deepx_return_host), so neither may the kernels"""
    v = V["RET130"]
    got = _render_x(fr, renderer, v, w=W, h=H)
    want = _render_plain(fr, renderer, v, w=W, h=H)
    for plane, g, w_ in zip(("rgba", "nu", "iter"), got, want):
        assert np.array_equal(g.view(np.uint8), w_.view(np.uint8)), plane
    assert len(np.unique(got[2])) >= 100


@pytest.mark.parametrize("name", RET.NAMES)
def test_bla_planes_and_step_counts_are_the_restatement(fr, renderer, oracle, name):
    v = V[name]
    got = _render_x(fr, renderer, v, w=W, h=H, xbla=True)
    steps = tuple(renderer.last_deepx_steps())
    counts = tuple(RET.golden(name, "bla_counts").tolist())
    print(name, "counts", steps, "restated", counts)
    _check_planes(oracle, v, got, [(RET.golden(name, "bla_iter"), RET.golden(name, "bla_r2"))], 1, False)
    _check_exact(name, got[2])
    assert steps == counts and counts[1] > 0
    if name == "RET130":                                           # what the two restatements give: no pixel differs
        assert np.array_equal(RET.golden(name, "bla_iter"), RET.golden(name, "iter"))
        assert np.array_equal(got[2], _render_x(fr, renderer, v, w=W, h=H)[2])


@pytest.mark.parametrize("bla", [False, True], ids=["plain", "bla"])
@pytest.mark.parametrize("name", RET.NAMES)
def test_distance_estimate_planes_are_the_restatement(fr, renderer, name, bla):
    """the checks of test_deepx_de_gpu.test_planes_match_the_restatement_and_fr_render_deepx: deriv and iter bit for bit, de
    within 2^-50 relative, rgba, nu and iter the bytes of fr_render_deepx"""
    v = V[name]
    it, r2, Dx, Dy, eD = (RET.golden(name, ("debla_" if bla else "de_") + k) for k in ("iter", "r2", "Dx", "Dy", "eD"))
    got = _render_de(fr, renderer, v, W, H, bla=bla)
    steps = tuple(renderer.last_deepx_steps()) if bla else None
    assert np.array_equal(got["iter"], it), int((got["iter"] != it).sum())
    _check_exact(name, got["iter"])
    assert _same_bytes(got["deriv"], XD.deriv_of_x(it, Dx, Dy, eD, v["max_iter"]))
    _check_de(got["de"], XD.de_of_x(it, r2, Dx, Dy, eD, v["max_iter"]))
    esc = it < v["max_iter"]
    assert esc.sum() >= W * H - 1 and np.all(np.isfinite(got["de"])) and np.all(got["de"][esc] > 0.0)
    assert np.all(got["de"][~esc] == 0.0) and not got["deriv"][~esc].any()
    if bla:
        assert steps == tuple(RET.golden(name, "debla_counts").tolist()) and steps[1] > 0
    base = _render_x(fr, renderer, v, w=W, h=H, xbla=bla)
    for k, b in zip(("rgba", "nu", "iter"), base):
        assert _same_bytes(got[k], b), k


@pytest.mark.parametrize("name", RET.NAMES)
def test_phoenix_kernel_at_p_r_zero(fr, renderer, name):
    """the Phoenix loop's own plain-to-extended block, dq normalised with dz, on the Mandelbrot recurrence"""
    v = dict(V[name], p=0.0, r=0.0)
    _, nu, it = _render_phoenix(fr, renderer, v, w=W, h=H)
    r_it = RET.golden(name, "px_iter")
    print(name, "pixels that differ from the restatement", int((it != r_it).sum()))
    assert np.array_equal(it, r_it)
    _check_exact(name, it, phoenix=True)
    assert np.abs(nu - D.smooth(r_it, RET.golden(name, "px_zx"), RET.golden(name, "px_zy"), v["max_iter"])).max() <= PX_NU_TOL


@functools.lru_cache(maxsize=None)
def _ragged_samples():
    """the four sub-samples of RET130 at 31 x 23, aa 2, restated in one pass (about 20 s of CPU): computed once, never changed"""
    v = V["RET130"]
    w, h = RAGGED
    zm, ze = X.zoom_pair(v["zoom"])
    dcs = [X.sample_dc_x(w, h, zm, ze, 2, s) for s in range(4)]
    st = {}
    it, r2 = X.perturb_x(*X.orbit_of(v), tuple(np.concatenate([d[k] for d in dcs]) for k in range(5)), v["max_iter"], stats=st)
    return [(it.reshape(4, h, w)[s], r2.reshape(4, h, w)[s]) for s in range(4)], st


def test_ragged_frame_with_aa_2_and_the_post_chain(fr, renderer, oracle):
    w, h = RAGGED
    samples, st = _ragged_samples()
    print("RET130", RAGGED, st)
    assert st["to_ext"] >= 20 * 4 * w * h
    got = _render_x(fr, renderer, V["RET130"], 2, True, w=w, h=h)
    _check_planes(oracle, V["RET130"], got, samples, 2, True)
