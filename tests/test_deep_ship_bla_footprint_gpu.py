"""The store footprint of deep_kernel<Ship, BLA> (fr_render_deep_ship with FR_FLAG_DEEP_SHIP_BLA): guard-banded planes
(tests/guarded.py) around view SHIP_B at sizes from one pixel to several sub-tile rows, edges that are no sub-tile multiples
included -- (a) no byte outside the planes is touched, (b) no in-frame pixel stays unwritten, (c) what is written equals the
numpy restatement, the step counts included -- for whole frames and for one part of a 3-part sharding, packed and written in
place into whole-frame planes whose other rows stay untouched."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_ship_bla_ref as SB
import deep_ship_ref as S
from guarded import GuardedPlanes

pytestmark = pytest.mark.gpu

VIEW = S.SHIP_B
NU_TOL = 1e-9
SIZES = [(1, 1), (7, 5), (64, 48), (203, 117)]


@functools.lru_cache(maxsize=None)
def _orbit():
    return S.reference_orbit(VIEW["cx"], VIEW["cy"], VIEW["zoom"], VIEW["max_iter"])


@functools.lru_cache(maxsize=None)
def _reference(W, H):
    """computed once per size, shared, never changed"""
    ((it, r2),), counts = SB.restate_bla(VIEW, W, H, orbit=_orbit())
    return it, r2, tuple(counts)


@functools.lru_cache(maxsize=None)
def _reference_counts(W, H, rows):
    """the counts of a part: those of its rows (dcmax stays the whole frame's)"""
    return tuple(SB.restate_bla(VIEW, W, H, orbit=_orbit(), rows=list(rows))[1])


def _state(fr):
    return fr.FractalState(zoom=VIEW["zoom"], max_iterations=VIEW["max_iter"])


def _check(W, H, rows, nu, it):
    r_it, r_r2, _ = _reference(W, H)
    if it is not None:
        assert np.array_equal(it, r_it[rows]), int((it != r_it[rows]).sum())
    if nu is not None:
        assert np.abs(nu - S.smooth(r_it[rows], r_r2[rows], VIEW["max_iter"])).max() <= NU_TOL


@pytest.mark.parametrize("backend", ["device", "host"])
@pytest.mark.parametrize("geom", SIZES, ids=lambda g: "%dx%d" % g)
def test_whole_frame(fr, renderer, geom, backend):
    W, H = geom
    gp = GuardedPlanes(H, W, f64=True, backend=backend)
    renderer.render_deep_ship(_state(fr), W, H, fr.DeepView(VIEW["cx"], VIEW["cy"]), bla=True, **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0, {k: p.unwritten() for k, p in gp.present()}
    rgba, nu, it = gp.values()
    assert np.all(rgba[..., 3] == 1.0)
    _check(W, H, np.arange(H), nu, it)
    assert tuple(renderer.last_deep_ship_steps()) == _reference(W, H)[2]


@pytest.mark.parametrize("geom", SIZES[1:], ids=lambda g: "%dx%d" % g)
def test_packed_shard(fr, renderer, geom):
    """part 1 of 3 into planes of its own rows"""
    W, H = geom
    shard = fr.Shard(1, 3, 2 if H < 16 else 8)
    g = shard.global_rows(H)
    assert 0 < len(g) < H
    gp = GuardedPlanes(len(g), W, f64=True, backend="device")
    renderer.render_deep_ship(_state(fr), W, H, fr.DeepView(VIEW["cx"], VIEW["cy"]), shard=shard, bla=True, **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0
    _, nu, it = gp.values()
    _check(W, H, g, nu, it)
    assert tuple(renderer.last_deep_ship_steps()) == _reference_counts(W, H, tuple(int(y) for y in g))


@pytest.mark.parametrize("geom", SIZES[1:], ids=lambda g: "%dx%d" % g)
def test_three_part_shard_in_frame_layout(fr, renderer, geom):
    """part 1 of 3 alone into pattern-filled whole-frame planes, then the others"""
    W, H = geom
    E = fr._capi
    gp = GuardedPlanes(H, W, f64=True, backend="device")
    out = gp.output(E, E.FR_LAYOUT_FRAME)
    p = _state(fr).to_params(fr.FractalType.BurningShip, fr.Precision.F64, False)
    p.flags |= E.FR_FLAG_DEEP_SHIP_BLA
    cv = fr.DeepView(VIEW["cx"], VIEW["cy"]).to_c()
    strip = 2 if H < 16 else 8
    for part in (1, 0, 2):
        shard = fr.Shard(part, 3, strip)
        g = shard.global_rows(H)
        sh = shard.to_c()
        assert fr.lib().fr_render_deep_ship(renderer._ctx, C.byref(p), C.byref(cv), W, H, C.byref(sh), C.byref(out)) == E.FR_OK
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
