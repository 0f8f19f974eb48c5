"""The store footprint of deep_phoenix_kernel (fr_render_deep_phoenix, around view PA30) and of deep_phoenix_x_kernel
(fr_render_deepx_phoenix, around view PX400A): guard-banded planes (tests/guarded.py) at sizes from one pixel to several
sub-tile rows, edges that are no sub-tile multiples included -- (a) no byte outside the planes is touched, (b) no in-frame pixel
stays unwritten, (c) what is written equals the numpy restatement -- for whole frames, for each plane alone, and for row strips:
one part of a 3-part sharding, packed and written in place into whole-frame planes whose other rows stay untouched."""
import functools

import numpy as np
import pytest

import deep_phoenix_entries as PE
import deep_phoenix_ref as D
import deepx_phoenix_ref as DX
from guarded import GuardedPlanes

pytestmark = pytest.mark.gpu

NU_TOL = 1e-9
FP64 = PE.fp64(D.PA30, [(1, 1), (7, 5), (48, 36), (71, 53)])
# 8 x 8 sub-tiles: one, a part of one, 3 x 3 and 5 x 4 with ragged tails
EXT = PE.extended(DX.PX400A, [(1, 1), (7, 5), (21, 19), (37, 29)])
ENTRIES = [FP64, EXT]
ORBIT = {FP64: D.view_orbit, EXT: DX.orbit_of}
RESTATE = {FP64: D.restate, EXT: DX.restate_x}


@functools.lru_cache(maxsize=None)
def _orbit(entry):
    return ORBIT[entry](entry.view)


@functools.lru_cache(maxsize=None)
def _reference(entry, W, H):
    """computed once per entry and size, shared, never changed"""
    return RESTATE[entry](entry.view, W, H, orbit=_orbit(entry))[:2]


def _check(entry, W, H, rows, nu, it):
    r_it, r_nu = _reference(entry, W, H)
    if it is not None:
        assert np.array_equal(it, r_it[rows]), int((it != r_it[rows]).sum())
    if nu is not None:
        assert np.abs(nu - r_nu[rows]).max() <= NU_TOL


@pytest.mark.parametrize("backend", ["device", "host"])
@pytest.mark.parametrize("entry,geom", PE.cases(ENTRIES), ids=PE.case_id)
def test_whole_frame(fr, renderer, entry, geom, backend):
    W, H = geom
    gp = GuardedPlanes(H, W, f64=True, backend=backend)
    entry.render(fr, renderer, W, H, **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0, {k: p.unwritten() for k, p in gp.present()}
    rgba, nu, it = gp.values()
    assert np.all(rgba[..., 3] == 1.0)
    _check(entry, W, H, np.arange(H), nu, it)


@pytest.mark.parametrize("plane", GuardedPlanes.NAMES)
@pytest.mark.parametrize("entry,geom", PE.cases(ENTRIES, first=3), ids=PE.case_id)
def test_each_plane_alone(fr, renderer, entry, geom, plane):
    W, H = geom
    gp = GuardedPlanes(H, W, f64=True, backend="device", planes=(plane,))
    entry.render(fr, renderer, W, H, **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0
    rgba, nu, it = gp.values()
    _check(entry, W, H, np.arange(H), nu, it)
    if rgba is not None:
        assert np.all(rgba[..., 3] == 1.0)


@pytest.mark.parametrize("entry,geom", PE.cases(ENTRIES, first=1), ids=PE.case_id)
def test_packed_row_strips(fr, renderer, entry, geom):
    """part 1 of 3 into planes of its own rows"""
    W, H = geom
    shard = fr.Shard(1, 3, 2 if H < 16 else 8)
    g = shard.global_rows(H)
    assert 0 < len(g) < H
    gp = GuardedPlanes(len(g), W, f64=True, backend="device")
    entry.render(fr, renderer, W, H, shard=shard, **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0
    _, nu, it = gp.values()
    _check(entry, W, H, g, nu, it)


@pytest.mark.parametrize("entry,geom", PE.cases(ENTRIES, first=1), ids=PE.case_id)
def test_row_strips_in_frame_layout(fr, renderer, entry, geom):
    """part 1 of 3 alone into pattern-filled whole-frame planes, then the others"""
    W, H = geom
    E = fr._capi
    gp = GuardedPlanes(H, W, f64=True, backend="device")
    out = gp.output(E, E.FR_LAYOUT_FRAME)
    strip = 2 if H < 16 else 8
    for part in (1, 0, 2):
        shard = fr.Shard(part, 3, strip)
        g = shard.global_rows(H)
        assert entry.render_c(fr, renderer, W, H, shard, out) == E.FR_OK
        if part == 1:
            mine = np.zeros(H, bool)
            mine[g] = True
            assert mine.any() and not mine.all()
            assert gp.guards_intact(), gp.guard_hits()
            assert gp.unwritten(mine) == 0
            assert gp.untouched(~mine)
            _, nu, it = gp.values()
            _check(entry, W, H, g, nu[g], it[g])
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0
    _, nu, it = gp.values()
    _check(entry, W, H, np.arange(H), nu, it)
