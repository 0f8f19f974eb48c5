"""The store footprint of deep_kernel<Mandel, X, BLA> (fr_render_deepx with FR_FLAG_DEEPX_BLA): guard-banded planes
(tests/guarded.py) around view T320 at sizes from one pixel to several sub-tile rows -- (a) no byte outside the planes is
touched, (b) no in-frame pixel stays unwritten, (c) what is written equals the numpy restatement -- for whole frames, and
for one part of a 3-part sharding written in place into whole-frame planes, whose other rows stay untouched."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_ref as R
import deepx_bla_ref as XB
import deepx_ref as X
from guarded import GuardedPlanes
from test_deep_gpu import NU_TOL

pytestmark = pytest.mark.gpu

VIEW = X.views()["T320"]
SIZES = [(1, 1), (7, 5), (64, 48), (203, 117)]


@functools.lru_cache(maxsize=None)
def _orbit():
    return X.orbit_of(VIEW)


@functools.lru_cache(maxsize=None)
def _reference(W, H):
    """computed once per size, shared, never changed"""
    return XB.restate_x_bla(VIEW, W, H, orbit=_orbit())


def _check(W, H, rows, nu, it):
    (r_it, r_r2), = _reference(W, H)[0]
    assert np.array_equal(it, r_it[rows]), int((it != r_it[rows]).sum())
    assert np.abs(nu - R.smooth(r_it[rows], r_r2[rows], VIEW["max_iter"])).max() <= NU_TOL


@pytest.mark.parametrize("backend", ["device", "host"])
@pytest.mark.parametrize("geom", SIZES, ids=lambda g: "%dx%d" % g)
def test_whole_frame(fr, renderer, geom, backend):
    W, H = geom
    gp = GuardedPlanes(H, W, f64=True, backend=backend)
    renderer.render_deep(fr.FractalState(max_iterations=VIEW["max_iter"]), W, H,
                         fr.DeepView(VIEW["cx"], VIEW["cy"], zoom=VIEW["zoom"]), xbla=True, **gp.kwargs())
    assert tuple(renderer.last_deepx_steps()) == tuple(_reference(W, H)[1])
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0, {k: p.unwritten() for k, p in gp.present()}
    rgba, nu, it = gp.values()
    assert np.all(rgba[..., 3] == 1.0)
    _check(W, H, np.arange(H), nu, it)


@pytest.mark.parametrize("geom", SIZES[1:], ids=lambda g: "%dx%d" % g)
def test_three_part_shard_in_frame_layout(fr, renderer, geom):
    """part 1 of 3 alone into pattern-filled whole-frame planes, then the others"""
    W, H = geom
    E = fr._capi
    gp = GuardedPlanes(H, W, f64=True, backend="device")
    out = gp.output(E, E.FR_LAYOUT_FRAME)
    p = fr.FractalState(max_iterations=VIEW["max_iter"]).to_params(fr.FractalType.Mandelbrot, fr.Precision.F64, False)
    p.flags |= fr.FR_FLAG_DEEPX_BLA
    cv = fr.DeepView(VIEW["cx"], VIEW["cy"], zoom=VIEW["zoom"]).to_cx()
    strip = 2 if H < 16 else 8
    total = np.zeros(3, np.int64)
    for part in (1, 0, 2):
        shard = fr.Shard(part, 3, strip)
        g = shard.global_rows(H)
        sh = shard.to_c()
        assert fr.lib().fr_render_deepx(renderer._ctx, C.byref(p), C.byref(cv), W, H, C.byref(sh), C.byref(out)) == E.FR_OK
        if len(g):
            total += np.array(renderer.last_deepx_steps())
        if part == 1:
            mine = np.zeros(H, bool)
            mine[g] = True
            assert mine.any() and not mine.all()
            assert gp.guards_intact(), gp.guard_hits()
            assert gp.unwritten(mine) == 0
            assert gp.untouched(~mine)
            _, nu, it = gp.values()
            _check(W, H, g, nu[g], it[g])
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0
    _, nu, it = gp.values()
    _check(W, H, np.arange(H), nu, it)
    assert tuple(total) == tuple(_reference(W, H)[1])
