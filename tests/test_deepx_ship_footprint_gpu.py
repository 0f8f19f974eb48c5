"""The store footprint of deep_kernel<Ship, X> (fr_render_deepx_ship): guard-banded planes (tests/guarded.py) around
the tip view at 1e-400 at sizes from one pixel to several sub-tile rows, edges that are no sub-tile multiples included --
(a) no byte outside the planes is touched, (b) no in-frame pixel stays unwritten, (c) what is written equals the numpy
restatement -- for whole frames, for every subset of the planes, and for one part of a 3-part sharding, packed and written
in place into whole-frame planes whose other rows stay untouched."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import deep_ship_ref as S
import deepx_ship_ref as SX
from guarded import GuardedPlanes

pytestmark = pytest.mark.gpu

VIEW = SX.views()["TIP400"]
NU_TOL = 1e-9
SIZES = [(1, 1), (7, 5), (75, 53)]
SUBSETS = [c for n in (1, 2, 3) for c in itertools.combinations(GuardedPlanes.NAMES, n)]


@functools.lru_cache(maxsize=None)
def _orbit():
    return SX.orbit_of(VIEW)


@functools.lru_cache(maxsize=None)
def _reference(W, H):
    """computed once per size, shared, never changed"""
    (it, r2), = SX.restate_ship_x(VIEW, W, H, orbit=_orbit())
    return it, r2


def _state(fr):
    return fr.FractalState(max_iterations=VIEW["max_iter"])


def _view(fr):
    return fr.DeepView(VIEW["cx"], VIEW["cy"], zoom=VIEW["zoom"])


def _check(W, H, rows, nu, it):
    r_it, r_r2 = _reference(W, H)
    if it is not None:
        assert np.array_equal(it, r_it[rows]), int((it != r_it[rows]).sum())
    if nu is not None:
        assert np.abs(nu - S.smooth(r_it[rows], r_r2[rows], VIEW["max_iter"])).max() <= NU_TOL


@pytest.mark.parametrize("backend", ["device", "host"])
@pytest.mark.parametrize("geom", SIZES, ids=lambda g: "%dx%d" % g)
def test_whole_frame(fr, renderer, geom, backend):
    W, H = geom
    gp = GuardedPlanes(H, W, f64=True, backend=backend)
    renderer.render_deepx_ship(_state(fr), W, H, _view(fr), **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0, {k: p.unwritten() for k, p in gp.present()}
    rgba, nu, it = gp.values()
    assert np.all(rgba[..., 3] == 1.0)
    _check(W, H, np.arange(H), nu, it)


@pytest.mark.parametrize("planes", SUBSETS, ids=lambda s: "+".join(s))
def test_every_plane_subset(fr, renderer, planes):
    W, H = SIZES[-1]
    gp = GuardedPlanes(H, W, f64=True, backend="device", planes=planes)
    renderer.render_deepx_ship(_state(fr), W, H, _view(fr), **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0
    rgba, nu, it = gp.values()
    _check(W, H, np.arange(H), nu, it)
    if rgba is not None:
        assert np.all(rgba[..., 3] == 1.0)


@pytest.mark.parametrize("geom", SIZES[1:], ids=lambda g: "%dx%d" % g)
def test_packed_shard(fr, renderer, geom):
    """part 1 of 3 into planes of its own rows"""
    W, H = geom
    shard = fr.Shard(1, 3, 2 if H < 16 else 8)
    g = shard.global_rows(H)
    assert 0 < len(g) < H
    gp = GuardedPlanes(len(g), W, f64=True, backend="device")
    renderer.render_deepx_ship(_state(fr), W, H, _view(fr), shard=shard, **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0
    _, nu, it = gp.values()
    _check(W, H, g, nu, it)


@pytest.mark.parametrize("geom", SIZES[1:], ids=lambda g: "%dx%d" % g)
def test_three_part_shard_in_frame_layout(fr, renderer, geom):
    """part 1 of 3 alone into pattern-filled whole-frame planes, then the others"""
    W, H = geom
    E = fr._capi
    gp = GuardedPlanes(H, W, f64=True, backend="device")
    out = gp.output(E, E.FR_LAYOUT_FRAME)
    p = _state(fr).to_params(fr.FractalType.BurningShip, fr.Precision.F64, False)
    cv = _view(fr).to_cx()
    strip = 2 if H < 16 else 8
    for part in (1, 0, 2):
        shard = fr.Shard(part, 3, strip)
        g = shard.global_rows(H)
        sh = shard.to_c()
        assert fr.lib().fr_render_deepx_ship(renderer._ctx, C.byref(p), C.byref(cv), W, H, C.byref(sh), C.byref(out)) == E.FR_OK
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
