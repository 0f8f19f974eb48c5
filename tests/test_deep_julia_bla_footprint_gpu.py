"""The store footprint of deep_kernel<Julia, BLA> and deep_kernel<Julia, X, BLA> (fr_render_deep_julia with
FR_FLAG_DEEP_JULIA_BLA, fr_render_deepx_julia with FR_FLAG_DEEPX_JULIA_BLA) and of the table read-back: guard-banded planes
(tests/guarded.py) around view PRECRIT60, whose samples step on both tables, at sizes from one pixel to several sub-tile rows
with edges that are no sub-tile multiples -- (a) no byte outside the planes is touched, (b) no in-frame pixel stays unwritten,
(c) what is written equals the numpy restatement -- for whole frames and for one part of a 3-part sharding written in place
into whole-frame planes whose other rows stay untouched.  fr_deep_julia_bla_table / fr_deepx_julia_bla_table write into
guard-banded host arrays: exactly the entries asked for, equal to numpy's, which a level kernel's store past an entry's 24 or
28 bytes would break."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_julia_bla_ref as JB
import deep_julia_ref as J
from guarded import GuardedPlanes

pytestmark = pytest.mark.gpu

VIEW = JB.view("PRECRIT60")
NU_TOL = 1e-9
SIZES = [(1, 1), (7, 5), (64, 48), (203, 117)]
KERNELS = ["fp64", "extended"]
GUARD = 64                                                         # entries on either side of a read-back array


@functools.lru_cache(maxsize=None)
def _reference(W, H, kernel):
    """computed once per size and kernel, shared, never changed"""
    if kernel == "extended":
        return JB.restate_x_bla(VIEW, W, H, orbits=JB.orbits_x("PRECRIT60"))
    return JB.restate_bla(VIEW, W, H, orbits=JB.orbits("PRECRIT60"))


def _state(fr, kernel):
    return fr.FractalState(zoom=2.5 if kernel == "extended" else VIEW["zoom"], max_iterations=VIEW["max_iter"],
                           julia_c_real=VIEW["c"][0], julia_c_imag=VIEW["c"][1])


def _deep_view(fr, kernel):
    return fr.DeepView(VIEW["cx"], VIEW["cy"], zoom=VIEW["zoom_s"] if kernel == "extended" else None)


def _steps(renderer, kernel):
    return tuple(renderer.last_deepx_julia_steps() if kernel == "extended" else renderer.last_deep_julia_steps())


def _check(W, H, kernel, rows, nu, it):
    (r_it, r_r2), = _reference(W, H, kernel)[0]
    assert np.array_equal(it, r_it[rows]), int((it != r_it[rows]).sum())
    assert np.abs(nu - J.smooth(r_it[rows], r_r2[rows], VIEW["max_iter"])).max() <= NU_TOL


def _guarded(n, dtype, fill, guard=GUARD):
    a = np.empty(n + 2 * guard, dtype)
    a.view(np.uint8)[:] = fill
    return a


def _check_table(fr, renderer, kernel):
    """the read-back into guard-banded arrays: n entries written, the bands on both sides as they were"""
    L = fr.lib()
    if kernel == "extended":
        want_rv, want_re, want_a, want_e = JB.flat_x(JB.bla_tables_x(*JB.orbits_x("PRECRIT60")))
        n = len(want_rv)
        r = _guarded(n, np.dtype([("v", np.float32), ("e", np.int32)]), 0xA5)
        a = _guarded(2 * n, np.float64, 0xA5, 2 * GUARD)
        e = _guarded(n, np.int32, 0xA5)
        assert L.fr_deepx_julia_bla_table(renderer._ctx, r[GUARD:].ctypes.data, a[2 * GUARD:].ctypes.data, e[GUARD:].ctypes.data, n) == n
        assert np.array_equal(r["v"][GUARD:-GUARD].view(np.uint32), want_rv.view(np.uint32))
        assert np.array_equal(r["e"][GUARD:-GUARD], want_re) and np.array_equal(e[GUARD:-GUARD], want_e)
        bands = (r, e)
    else:
        want_r, want_a = JB.flat(JB.bla_tables(*JB.orbits("PRECRIT60")))
        n = len(want_r)
        r = _guarded(n, np.float64, 0xA5)
        a = _guarded(2 * n, np.float64, 0xA5, 2 * GUARD)
        assert L.fr_deep_julia_bla_table(renderer._ctx, r[GUARD:].ctypes.data, a[2 * GUARD:].ctypes.data, n) == n
        assert np.array_equal(r[GUARD:-GUARD].view(np.uint64), want_r.view(np.uint64))
        bands = (r,)
    P, Q = JB.orbits("PRECRIT60")                                  # Q runs to max_iter, P leaves the dendrite after 300 or so
    assert n == JB.entries(len(Q) - 1) + JB.entries(len(P) - 1) and len(Q) - 1 == VIEW["max_iter"] > len(P) - 1 > 256
    assert np.array_equal(a[2 * GUARD:-2 * GUARD].view(np.uint64), np.ascontiguousarray(want_a).ravel().view(np.uint64))
    for arr, g in [(b, GUARD) for b in bands] + [(a, 2 * GUARD)]:
        raw = arr.view(np.uint8)
        gb = g * arr.dtype.itemsize
        assert (raw[:gb] == 0xA5).all() and (raw[-gb:] == 0xA5).all()
    # fewer entries than the table has: those and no more
    m = n // 3
    r2 = _guarded(m, r.dtype, 0x5A)
    if kernel == "extended":
        assert L.fr_deepx_julia_bla_table(renderer._ctx, r2[GUARD:].ctypes.data, None, None, m) == n
    else:
        assert L.fr_deep_julia_bla_table(renderer._ctx, r2[GUARD:].ctypes.data, None, m) == n
    assert np.array_equal(r2[GUARD:-GUARD].view(np.uint8), r[GUARD:GUARD + m].view(np.uint8))
    gb = GUARD * r.dtype.itemsize
    assert (r2.view(np.uint8)[:gb] == 0x5A).all() and (r2.view(np.uint8)[-gb:] == 0x5A).all()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("backend", ["device", "host"])
@pytest.mark.parametrize("geom", SIZES, ids=lambda g: "%dx%d" % g)
def test_whole_frame(fr, renderer, geom, backend, kernel):
    W, H = geom
    gp = GuardedPlanes(H, W, f64=True, backend=backend)
    renderer.render_deep_julia(_state(fr, kernel), W, H, _deep_view(fr, kernel), bla=True, **gp.kwargs())
    assert _steps(renderer, kernel) == tuple(_reference(W, H, kernel)[1])
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0, {k: p.unwritten() for k, p in gp.present()}
    rgba, nu, it = gp.values()
    assert np.all(rgba[..., 3] == 1.0)
    _check(W, H, kernel, np.arange(H), nu, it)
    if geom == SIZES[-1] and backend == "device":
        _check_table(fr, renderer, kernel)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("geom", SIZES[1:], ids=lambda g: "%dx%d" % g)
def test_three_part_shard_in_frame_layout(fr, renderer, geom, kernel):
    """part 1 of 3 alone into pattern-filled whole-frame planes, then the others"""
    W, H = geom
    E = fr._capi
    gp = GuardedPlanes(H, W, f64=True, backend="device")
    out = gp.output(E, E.FR_LAYOUT_FRAME)
    p = _state(fr, kernel).to_params(fr.FractalType.JuliaSet, fr.Precision.F64, False)
    p.flags |= fr.FR_FLAG_DEEPX_JULIA_BLA if kernel == "extended" else fr.FR_FLAG_DEEP_JULIA_BLA
    dv = _deep_view(fr, kernel)
    cv = dv.to_cx() if kernel == "extended" else dv.to_c()
    entry = fr.lib().fr_render_deepx_julia if kernel == "extended" else fr.lib().fr_render_deep_julia
    strip = 2 if H < 16 else 8
    total = np.zeros(3, np.int64)
    for part in (1, 0, 2):
        shard = fr.Shard(part, 3, strip)
        g = shard.global_rows(H)
        sh = shard.to_c()
        assert entry(renderer._ctx, C.byref(p), C.byref(cv), W, H, C.byref(sh), C.byref(out)) == E.FR_OK
        if len(g):
            total += np.array(_steps(renderer, kernel))
        if part == 1:
            mine = np.zeros(H, bool)
            mine[g] = True
            assert mine.any() and not mine.all()
            assert gp.guards_intact(), gp.guard_hits()
            assert gp.unwritten(mine) == 0
            assert gp.untouched(~mine)
            _, nu, it = gp.values()
            _check(W, H, kernel, g, nu[g], it[g])
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0
    _, nu, it = gp.values()
    _check(W, H, kernel, np.arange(H), nu, it)
    assert tuple(total) == tuple(_reference(W, H, kernel)[1])
