"""The store footprint of deep_phoenix_x_kernel (fr_render_deepx_phoenix): guard-banded planes (tests/guarded.py) around view PX400A at
sizes from one pixel to several sub-tile rows, edges that are no sub-tile multiples included -- (a) no byte outside the planes
is touched, (b) no in-frame pixel stays unwritten, (c) what is written equals the numpy restatement -- for whole frames, for
each plane alone, and for row strips: one part of a 3-part sharding, packed and written in place into whole-frame planes whose
other rows stay untouched."""
import ctypes as C
import functools

import numpy as np
import pytest

import deepx_phoenix_ref as D
from guarded import GuardedPlanes

pytestmark = pytest.mark.gpu

VIEW = D.PX400A
NU_TOL = 1e-9
SIZES = [(1, 1), (7, 5), (21, 19), (37, 29)]     # 8 x 8 sub-tiles: one, a part of one, 3 x 3 and 5 x 4 with ragged tails


@functools.lru_cache(maxsize=None)
def _orbit():
    return D.orbit_of(VIEW)


@functools.lru_cache(maxsize=None)
def _reference(W, H):
    """computed once per size, shared, never changed"""
    it, nu, _ = D.restate_x(VIEW, W, H, orbit=_orbit())
    return it, nu


def _state(fr):
    return fr.FractalState(max_iterations=VIEW["max_iter"])


def _call(fr, renderer, W, H, **kw):
    renderer.render_deepx_phoenix(_state(fr), W, H, fr.DeepView(VIEW["cx"], VIEW["cy"], zoom=VIEW["zoom"]),
                                  fr.PhoenixParams(phoenix_p=VIEW["p"], phoenix_r=VIEW["r"]), **kw)


def _check(W, H, rows, nu, it):
    r_it, r_nu = _reference(W, H)
    if it is not None:
        assert np.array_equal(it, r_it[rows]), int((it != r_it[rows]).sum())
    if nu is not None:
        assert np.abs(nu - r_nu[rows]).max() <= NU_TOL


@pytest.mark.parametrize("backend", ["device", "host"])
@pytest.mark.parametrize("geom", SIZES, ids=lambda g: "%dx%d" % g)
def test_whole_frame(fr, renderer, geom, backend):
    W, H = geom
    gp = GuardedPlanes(H, W, f64=True, backend=backend)
    _call(fr, renderer, W, H, **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0, {k: p.unwritten() for k, p in gp.present()}
    rgba, nu, it = gp.values()
    assert np.all(rgba[..., 3] == 1.0)
    _check(W, H, np.arange(H), nu, it)


@pytest.mark.parametrize("plane", GuardedPlanes.NAMES)
def test_each_plane_alone(fr, renderer, plane):
    W, H = 37, 29
    gp = GuardedPlanes(H, W, f64=True, backend="device", planes=(plane,))
    _call(fr, renderer, W, H, **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0
    rgba, nu, it = gp.values()
    _check(W, H, np.arange(H), nu, it)
    if rgba is not None:
        assert np.all(rgba[..., 3] == 1.0)


@pytest.mark.parametrize("geom", SIZES[1:], ids=lambda g: "%dx%d" % g)
def test_packed_row_strips(fr, renderer, geom):
    """part 1 of 3 into planes of its own rows"""
    W, H = geom
    shard = fr.Shard(1, 3, 2 if H < 16 else 8)
    g = shard.global_rows(H)
    assert 0 < len(g) < H
    gp = GuardedPlanes(len(g), W, f64=True, backend="device")
    _call(fr, renderer, W, H, shard=shard, **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0
    _, nu, it = gp.values()
    _check(W, H, g, nu, it)


@pytest.mark.parametrize("geom", SIZES[1:], ids=lambda g: "%dx%d" % g)
def test_row_strips_in_frame_layout(fr, renderer, geom):
    """part 1 of 3 alone into pattern-filled whole-frame planes, then the others"""
    W, H = geom
    E = fr._capi
    gp = GuardedPlanes(H, W, f64=True, backend="device")
    out = gp.output(E, E.FR_LAYOUT_FRAME)
    p = _state(fr).to_params(fr.FractalType.Phoenix, fr.Precision.F64, False)
    cv = fr.DeepView(VIEW["cx"], VIEW["cy"], zoom=VIEW["zoom"]).to_cx()
    ph = fr.PhoenixParams(phoenix_p=VIEW["p"], phoenix_r=VIEW["r"]).to_c()
    strip = 2 if H < 16 else 8
    for part in (1, 0, 2):
        shard = fr.Shard(part, 3, strip)
        g = shard.global_rows(H)
        sh = shard.to_c()
        assert fr.lib().fr_render_deepx_phoenix(renderer._ctx, C.byref(p), C.byref(ph), C.byref(cv), W, H, C.byref(sh),
                                                C.byref(out)) == E.FR_OK
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
