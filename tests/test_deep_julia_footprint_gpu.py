"""The store footprint of deep_kernel<Julia> and deep_kernel<Julia, X> (fr_render_deep_julia,
fr_render_deepx_julia): guard-banded planes (tests/guarded.py) around view DENDRITE30 at sizes from one pixel to several
sub-tile rows, edges that are no sub-tile multiples included -- (a) no byte outside the planes is touched, (b) no in-frame
pixel stays unwritten, (c) what is written equals the numpy restatement -- for whole frames, for each plane alone, and for
one part of a 3-part sharding, packed and written in place into whole-frame planes whose other rows stay untouched."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_julia_ref as J
from guarded import GuardedPlanes

pytestmark = pytest.mark.gpu

VIEW = J.view("DENDRITE30")
NU_TOL = 1e-9
SIZES = [(1, 1), (7, 5), (64, 48), (203, 117)]
KERNELS = ["fp64", "extended"]


@functools.lru_cache(maxsize=None)
def _orbits():
    return J.reference_orbits(VIEW)


@functools.lru_cache(maxsize=None)
def _reference(W, H):
    """computed once per size, shared, never changed (the two kernels give the same bytes on this view)"""
    (it, r2), = J.restate(VIEW, W, H, orbits=_orbits())
    return it, r2


def _state(fr):
    return fr.FractalState(zoom=VIEW["zoom"], max_iterations=VIEW["max_iter"], julia_c_real=VIEW["c"][0], julia_c_imag=VIEW["c"][1])


def _deep_view(fr, kernel):
    return fr.DeepView(VIEW["cx"], VIEW["cy"], zoom=VIEW["zoom_s"] if kernel == "extended" else None)


def _check(W, H, rows, nu, it):
    r_it, r_r2 = _reference(W, H)
    if it is not None:
        assert np.array_equal(it, r_it[rows]), int((it != r_it[rows]).sum())
    if nu is not None:
        assert np.abs(nu - J.smooth(r_it[rows], r_r2[rows], VIEW["max_iter"])).max() <= NU_TOL


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("backend", ["device", "host"])
@pytest.mark.parametrize("geom", SIZES, ids=lambda g: "%dx%d" % g)
def test_whole_frame(fr, renderer, geom, backend, kernel):
    W, H = geom
    gp = GuardedPlanes(H, W, f64=True, backend=backend)
    renderer.render_deep_julia(_state(fr), W, H, _deep_view(fr, kernel), **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0, {k: p.unwritten() for k, p in gp.present()}
    rgba, nu, it = gp.values()
    assert np.all(rgba[..., 3] == 1.0)
    _check(W, H, np.arange(H), nu, it)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("plane", GuardedPlanes.NAMES)
def test_each_plane_alone(fr, renderer, plane, kernel):
    W, H = 203, 117
    gp = GuardedPlanes(H, W, f64=True, backend="device", planes=(plane,))
    renderer.render_deep_julia(_state(fr), W, H, _deep_view(fr, kernel), **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0
    rgba, nu, it = gp.values()
    _check(W, H, np.arange(H), nu, it)
    if rgba is not None:
        assert np.all(rgba[..., 3] == 1.0)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("geom", SIZES[1:], ids=lambda g: "%dx%d" % g)
def test_packed_shard(fr, renderer, geom, kernel):
    """part 1 of 3 into planes of its own rows"""
    W, H = geom
    shard = fr.Shard(1, 3, 2 if H < 16 else 8)
    g = shard.global_rows(H)
    assert 0 < len(g) < H
    gp = GuardedPlanes(len(g), W, f64=True, backend="device")
    renderer.render_deep_julia(_state(fr), W, H, _deep_view(fr, kernel), shard=shard, **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0
    _, nu, it = gp.values()
    _check(W, H, g, nu, it)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("geom", SIZES[1:], ids=lambda g: "%dx%d" % g)
def test_three_part_shard_in_frame_layout(fr, renderer, geom, kernel):
    """part 1 of 3 alone into pattern-filled whole-frame planes, then the others"""
    W, H = geom
    E = fr._capi
    gp = GuardedPlanes(H, W, f64=True, backend="device")
    out = gp.output(E, E.FR_LAYOUT_FRAME)
    p = _state(fr).to_params(fr.FractalType.JuliaSet, fr.Precision.F64, False)
    dv = _deep_view(fr, kernel)
    cv = dv.to_cx() if kernel == "extended" else dv.to_c()
    entry = fr.lib().fr_render_deepx_julia if kernel == "extended" else fr.lib().fr_render_deep_julia
    strip = 2 if H < 16 else 8
    for part in (1, 0, 2):
        shard = fr.Shard(part, 3, strip)
        g = shard.global_rows(H)
        sh = shard.to_c()
        assert entry(renderer._ctx, C.byref(p), C.byref(cv), W, H, C.byref(sh), C.byref(out)) == E.FR_OK
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
