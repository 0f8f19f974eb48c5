"""The store footprint of deep_kernel<Ship, X, BLA> and of the table build (fr_render_deepx_ship with
FR_FLAG_DEEPX_SHIP_BLA): guard-banded planes (tests/guarded.py) around view S400 at sizes from one pixel to several sub-tile
rows -- (a) no byte outside the planes is touched, (b) no in-frame pixel stays unwritten, (c) what is written equals the numpy
restatement -- for whole frames, and for one part of a 3-part sharding written in place into whole-frame planes, whose other
rows stay untouched.  Every size has a dcmax of its own, so every render here rebuilds the table next to the guarded planes;
the table itself is compared with numpy's entry for entry, which a store past an entry's 80 bytes would break."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_ship_ref as S
import deepx_ship_bla_ref as XB
import deepx_ship_ref as SX
from guarded import GuardedPlanes
from test_deepx_ship_gpu import NU_TOL

pytestmark = pytest.mark.gpu

VIEW = SX.views()["S400"]
SIZES = [(1, 1), (7, 5), (64, 48), (203, 117)]


@functools.lru_cache(maxsize=None)
def _orbit():
    return SX.orbit_of(VIEW)


@functools.lru_cache(maxsize=None)
def _reference(W, H):
    """computed once per size, shared, never changed"""
    return XB.restate_ship_x_bla(VIEW, W, H, orbit=_orbit())


def _check(W, H, rows, nu, it):
    (r_it, r_r2), = _reference(W, H)[0]
    assert np.array_equal(it, r_it[rows]), int((it != r_it[rows]).sum())
    assert np.abs(nu - S.smooth(r_it[rows], r_r2[rows], VIEW["max_iter"])).max() <= NU_TOL


def _check_table(fr, renderer, W, H):
    tab = XB.table_of(VIEW, W, H, _orbit())
    n = sum(len(T["rv"]) for T in tab)
    r = np.empty(n, np.dtype([("v", np.float32), ("e", np.int32)]))
    ab = np.empty((n, 8), np.float64)
    abe = np.empty((n, 2), np.int32)
    assert fr.lib().fr_deepx_ship_bla_table(renderer._ctx, r.ctypes.data, ab.ctypes.data, abe.ctypes.data, n) == n
    assert np.array_equal(r["v"], np.concatenate([T["rv"] for T in tab]).astype(np.float32))
    assert np.array_equal(r["e"], np.concatenate([T["re"] for T in tab]).astype(np.int32))
    assert np.array_equal(ab, np.concatenate([np.stack([T[q] for q in XB.ELEMS], axis=1) for T in tab]))
    assert np.array_equal(abe, np.concatenate([np.stack([T["ea"], T["eb"]], axis=1) for T in tab]).astype(np.int32))


@pytest.mark.parametrize("backend", ["device", "host"])
@pytest.mark.parametrize("geom", SIZES, ids=lambda g: "%dx%d" % g)
def test_whole_frame(fr, renderer, geom, backend):
    W, H = geom
    gp = GuardedPlanes(H, W, f64=True, backend=backend)
    renderer.render_deepx_ship(fr.FractalState(max_iterations=VIEW["max_iter"]), W, H,
                               fr.DeepView(VIEW["cx"], VIEW["cy"], zoom=VIEW["zoom"]), bla=True, **gp.kwargs())
    assert tuple(renderer.last_deepx_ship_steps()) == tuple(_reference(W, H)[1])
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0, {k: p.unwritten() for k, p in gp.present()}
    rgba, nu, it = gp.values()
    assert np.all(rgba[..., 3] == 1.0)
    _check(W, H, np.arange(H), nu, it)
    _check_table(fr, renderer, W, H)


@pytest.mark.parametrize("geom", SIZES[1:], ids=lambda g: "%dx%d" % g)
def test_three_part_shard_in_frame_layout(fr, renderer, geom):
    """part 1 of 3 alone into pattern-filled whole-frame planes, then the others"""
    W, H = geom
    E = fr._capi
    gp = GuardedPlanes(H, W, f64=True, backend="device")
    out = gp.output(E, E.FR_LAYOUT_FRAME)
    p = fr.FractalState(max_iterations=VIEW["max_iter"]).to_params(fr.FractalType.BurningShip, fr.Precision.F64, False)
    p.flags |= fr.FR_FLAG_DEEPX_SHIP_BLA
    cv = fr.DeepView(VIEW["cx"], VIEW["cy"], zoom=VIEW["zoom"]).to_cx()
    strip = 2 if H < 16 else 8
    total = np.zeros(3, np.int64)
    for part in (1, 0, 2):
        shard = fr.Shard(part, 3, strip)
        g = shard.global_rows(H)
        sh = shard.to_c()
        assert fr.lib().fr_render_deepx_ship(renderer._ctx, C.byref(p), C.byref(cv), W, H, C.byref(sh), C.byref(out)) == E.FR_OK
        if len(g):
            total += np.array(renderer.last_deepx_ship_steps())
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
