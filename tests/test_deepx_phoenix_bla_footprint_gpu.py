"""The store footprint of deep_phoenix_x_bla_kernel (fr_render_deepx_phoenix with FR_FLAG_DEEPX_PHOENIX_BLA) and of the table
read-back (fr_deepx_phoenix_bla_table): guard-banded planes (tests/guarded.py) around view PX310 at 40 x 24 and at a ragged size
whose edges are no sub-tile multiples -- (a) no byte outside the planes is touched, (b) no in-frame pixel stays unwritten,
(c) what is written equals the numpy restatement, the step counts included -- for whole frames and for one part of a 3-part
sharding, packed and written in place into whole-frame planes whose other rows stay untouched; and the read-back writes the
entries it was asked for, no more."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_phoenix_ref as D
import deepx_phoenix_bla_ref as XB
import deepx_phoenix_ref as PX
from guarded import F64_PATTERN, Guarded, GuardedPlanes

pytestmark = pytest.mark.gpu

VIEW = PX.PX310
NU_TOL = 1e-9                      # test_deep_phoenix_gpu.py's
SIZES = [(40, 24), (71, 53)]


@functools.lru_cache(maxsize=None)
def _orbit():
    return PX.orbit_of(VIEW)


@functools.lru_cache(maxsize=None)
def _reference(W, H):
    """computed once per size, shared, never changed"""
    ((it, _, zx, zy),), counts = XB.samples_x_bla(VIEW, W, H, orbit=_orbit())
    return it, D.smooth(it, zx, zy, VIEW["max_iter"]), tuple(counts)


@functools.lru_cache(maxsize=None)
def _reference_counts(W, H, rows):
    """the counts of a part: those of its rows (dcmax stays the whole frame's)"""
    return tuple(XB.samples_x_bla(VIEW, W, H, orbit=_orbit(), rows=list(rows))[1])


def _state(fr):
    return fr.FractalState(max_iterations=VIEW["max_iter"])


def _ph(fr):
    return fr.PhoenixParams(phoenix_p=VIEW["p"], phoenix_r=VIEW["r"])


def _dv(fr):
    return fr.DeepView(VIEW["cx"], VIEW["cy"], zoom=VIEW["zoom"])


def _check(W, H, rows, nu, it):
    r_it, r_nu, _ = _reference(W, H)
    assert np.array_equal(it, r_it[rows]), int((it != r_it[rows]).sum())
    assert np.abs(nu - r_nu[rows]).max() <= NU_TOL


@pytest.mark.parametrize("backend", ["device", "host"])
@pytest.mark.parametrize("geom", SIZES, ids=lambda g: "%dx%d" % g)
def test_whole_frame(fr, renderer, geom, backend):
    W, H = geom
    gp = GuardedPlanes(H, W, f64=True, backend=backend)
    renderer.render_deepx_phoenix(_state(fr), W, H, _dv(fr), _ph(fr), xbla=True, **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0, {k: p.unwritten() for k, p in gp.present()}
    rgba, nu, it = gp.values()
    assert np.all(rgba[..., 3] == 1.0)
    _check(W, H, np.arange(H), nu, it)
    steps = tuple(renderer.last_deepx_phoenix_steps())
    assert steps == _reference(W, H)[2] and steps[1] > 0


@pytest.mark.parametrize("geom", SIZES, ids=lambda g: "%dx%d" % g)
def test_packed_shard(fr, renderer, geom):
    """part 1 of 3 into planes of its own rows"""
    W, H = geom
    shard = fr.Shard(1, 3, 8)
    g = shard.global_rows(H)
    assert 0 < len(g) < H
    gp = GuardedPlanes(len(g), W, f64=True, backend="device")
    renderer.render_deepx_phoenix(_state(fr), W, H, _dv(fr), _ph(fr), shard=shard, xbla=True, **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0
    _, nu, it = gp.values()
    _check(W, H, g, nu, it)
    assert tuple(renderer.last_deepx_phoenix_steps()) == _reference_counts(W, H, tuple(int(y) for y in g))


@pytest.mark.parametrize("geom", SIZES, ids=lambda g: "%dx%d" % g)
def test_three_part_shard_in_frame_layout(fr, renderer, geom):
    """part 1 of 3 alone into pattern-filled whole-frame planes, then the others"""
    W, H = geom
    E = fr._capi
    gp = GuardedPlanes(H, W, f64=True, backend="device")
    out = gp.output(E, E.FR_LAYOUT_FRAME)
    p = _state(fr).to_params(fr.FractalType.Phoenix, fr.Precision.F64, False)
    p.flags |= E.FR_FLAG_DEEPX_PHOENIX_BLA
    cv = _dv(fr).to_cx()
    cph = _ph(fr).to_c()
    for part in (1, 0, 2):
        shard = fr.Shard(part, 3, 8)
        g = shard.global_rows(H)
        sh = shard.to_c()
        assert fr.lib().fr_render_deepx_phoenix(renderer._ctx, C.byref(p), C.byref(cph), C.byref(cv), W, H, C.byref(sh),
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


@pytest.mark.parametrize("ask", ["all", "some", "more"])
def test_table_read_back_writes_the_entries_asked_for(fr, renderer, ask):
    """fr_deepx_phoenix_bla_table into guarded host arrays: n entries of 8 bytes, 12 doubles and 2 int32, whatever the table
    holds"""
    W, H = SIZES[0]
    renderer.render_deepx_phoenix(_state(fr), W, H, _dv(fr), _ph(fr), xbla=True, iter=np.empty((H, W), np.int32))
    want_r, want_mb, want_e = XB.table_arrays(XB.view_table(VIEW, W, H, _orbit()))
    have = len(want_r)
    n = {"all": have, "some": 5, "more": have + 7}[ask]
    room = max(n, have)
    r = Guarded(room, np.float64, F64_PATTERN, 512)                  # 8 bytes per entry: the float and the int32
    mb = Guarded(room * XB.ENTRY_DOUBLES, np.float64, F64_PATTERN, 512)
    ex = Guarded(room, np.float64, F64_PATTERN, 512)                 # 2 int32 per entry
    got = fr.lib().fr_deepx_phoenix_bla_table(renderer._ctx, r.address(), mb.address(), ex.address(), n)
    assert got == have
    wrote = min(n, have)
    assert r.guards_intact() and mb.guards_intact() and ex.guards_intact()
    assert np.array_equal(r.payload_bits()[:wrote], np.ascontiguousarray(want_r).view(np.uint64).ravel()[:wrote])
    assert np.array_equal(mb.payload_bits()[:wrote * XB.ENTRY_DOUBLES], want_mb.view(np.uint64).ravel()[:wrote * XB.ENTRY_DOUBLES])
    assert np.array_equal(ex.payload_bits()[:wrote], np.ascontiguousarray(want_e).view(np.uint64).ravel()[:wrote])
    assert r.still_pattern()[wrote:].all() and mb.still_pattern()[wrote * XB.ENTRY_DOUBLES:].all()
    assert ex.still_pattern()[wrote:].all()
