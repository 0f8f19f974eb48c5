"""The store footprint of deep_phoenix_bla_kernel (fr_render_deep_phoenix with FR_FLAG_DEEP_PHOENIX_BLA, around view PA30) and of
deep_phoenix_x_bla_kernel (fr_render_deepx_phoenix with FR_FLAG_DEEPX_PHOENIX_BLA, around view PX310), and of the table read-backs
(fr_deep_phoenix_bla_table, fr_deepx_phoenix_bla_table): guard-banded planes (tests/guarded.py) at 40 x 24 and at a ragged size
whose edges are no sub-tile multiples -- (a) no byte outside the planes is touched, (b) no in-frame pixel stays unwritten,
(c) what is written equals the numpy restatement, the step counts included -- for whole frames and for one part of a 3-part
sharding, packed and written in place into whole-frame planes whose other rows stay untouched; and the read-back writes the
entries it was asked for, no more."""
import functools

import numpy as np
import pytest

import deep_phoenix_bla_ref as PB
import deep_phoenix_entries as PE
import deep_phoenix_ref as D
import deepx_phoenix_bla_ref as XB
import deepx_phoenix_ref as PX
from guarded import F64_PATTERN, Guarded, GuardedPlanes

pytestmark = pytest.mark.gpu

NU_TOL = 1e-9                      # test_deep_phoenix_gpu.py's
SIZES = [(40, 24), (71, 53)]
FP64 = PE.fp64(D.PA30, SIZES)
EXT = PE.extended(PX.PX310, SIZES)
ENTRIES = [FP64, EXT]
CASES = pytest.mark.parametrize("entry,geom", PE.cases(ENTRIES), ids=PE.case_id)
ORBIT = {FP64: D.view_orbit, EXT: PX.orbit_of}
SAMPLES = {FP64: PB.samples_bla, EXT: XB.samples_x_bla}
# the table of a view and frame as the arrays its read-back fills, 8-byte words per entry in each: the radius (fp64: a double;
# extended: the float and the int32), the 12 doubles of M and B, and with the extended storage their 2 int32 exponents
TABLE = {FP64: (PB, "fr_deep_phoenix_bla_table", (1, PB.ENTRY_DOUBLES)),
         EXT: (XB, "fr_deepx_phoenix_bla_table", (1, XB.ENTRY_DOUBLES, 1))}


@functools.lru_cache(maxsize=None)
def _orbit(entry):
    return ORBIT[entry](entry.view)


@functools.lru_cache(maxsize=None)
def _reference(entry, W, H):
    """computed once per entry and size, shared, never changed"""
    ((it, _, zx, zy),), counts = SAMPLES[entry](entry.view, W, H, orbit=_orbit(entry))
    return it, D.smooth(it, zx, zy, entry.view["max_iter"]), tuple(counts)


@functools.lru_cache(maxsize=None)
def _reference_counts(entry, W, H, rows):
    """the counts of a part: those of its rows (dcmax stays the whole frame's)"""
    return tuple(SAMPLES[entry](entry.view, W, H, orbit=_orbit(entry), rows=list(rows))[1])


def _check(entry, W, H, rows, nu, it):
    r_it, r_nu, _ = _reference(entry, W, H)
    assert np.array_equal(it, r_it[rows]), int((it != r_it[rows]).sum())
    assert np.abs(nu - r_nu[rows]).max() <= NU_TOL


@pytest.mark.parametrize("backend", ["device", "host"])
@CASES
def test_whole_frame(fr, renderer, entry, geom, backend):
    W, H = geom
    gp = GuardedPlanes(H, W, f64=True, backend=backend)
    entry.render(fr, renderer, W, H, **entry.bla_kw, **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0, {k: p.unwritten() for k, p in gp.present()}
    rgba, nu, it = gp.values()
    assert np.all(rgba[..., 3] == 1.0)
    _check(entry, W, H, np.arange(H), nu, it)
    steps = entry.last_steps(renderer)
    assert steps == _reference(entry, W, H)[2] and steps[1] > 0


@CASES
def test_packed_shard(fr, renderer, entry, geom):
    """part 1 of 3 into planes of its own rows"""
    W, H = geom
    shard = fr.Shard(1, 3, 8)
    g = shard.global_rows(H)
    assert 0 < len(g) < H
    gp = GuardedPlanes(len(g), W, f64=True, backend="device")
    entry.render(fr, renderer, W, H, shard=shard, **entry.bla_kw, **gp.kwargs())
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.unwritten() == 0
    _, nu, it = gp.values()
    _check(entry, W, H, g, nu, it)
    assert entry.last_steps(renderer) == _reference_counts(entry, W, H, tuple(int(y) for y in g))


@CASES
def test_three_part_shard_in_frame_layout(fr, renderer, entry, geom):
    """part 1 of 3 alone into pattern-filled whole-frame planes, then the others"""
    W, H = geom
    E = fr._capi
    gp = GuardedPlanes(H, W, f64=True, backend="device")
    out = gp.output(E, E.FR_LAYOUT_FRAME)
    for part in (1, 0, 2):
        shard = fr.Shard(part, 3, 8)
        g = shard.global_rows(H)
        assert entry.render_c(fr, renderer, W, H, shard, out, flags=getattr(E, entry.flag)) == E.FR_OK
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


@pytest.mark.parametrize("ask", ["all", "some", "more"])
@pytest.mark.parametrize("entry", ENTRIES, ids=repr)
def test_table_read_back_writes_the_entries_asked_for(fr, renderer, entry, ask):
    """the read-back into guarded host arrays: n entries in each of the table's arrays, whatever the table holds"""
    W, H = SIZES[0]
    ref, read_back, words = TABLE[entry]
    entry.render(fr, renderer, W, H, **entry.bla_kw, iter=np.empty((H, W), np.int32))
    want = [np.ascontiguousarray(a).view(np.uint64).ravel() for a in ref.table_arrays(ref.view_table(entry.view, W, H, _orbit(entry)))]
    have = len(want[0])
    n = {"all": have, "some": 5, "more": have + 7}[ask]
    room = max(n, have)
    got = [Guarded(room * k, np.float64, F64_PATTERN, 512) for k in words]
    assert getattr(fr.lib(), read_back)(renderer._ctx, *[a.address() for a in got], n) == have
    wrote = min(n, have)
    for a, w, k in zip(got, want, words):
        assert a.guards_intact()
        assert np.array_equal(a.payload_bits()[:wrote * k], w[:wrote * k])
        assert a.still_pattern()[wrote * k:].all()
