"""tests/guarded.py on numpy buffers: a correct store is clean under all three questions, and each kind of wrong store --
one element past the end, one before the start, one payload element left alone, one element in a foreign row -- is
reported.  The checker is shown to detect what it claims before any kernel is held to it."""
import numpy as np
import pytest

import guarded as G

ROWS, W = 13, 21
MINE = np.arange(ROWS) % 3 == 1              # the rows of "this part" in a whole-frame plane


def _planes(f64, planes=G.GuardedPlanes.NAMES):
    return G.GuardedPlanes(ROWS, W, f64=f64, backend="host", planes=planes)


def _store(gp, rows=None):
    """what a correct call does: every element of the rows it owns, NaN among the values"""
    rows = np.ones(ROWS, bool) if rows is None else rows
    for name, p in gp.present():
        v = p.payload(p.shape)
        v[rows] = (np.arange(v[rows].size).reshape(v[rows].shape) % 251).astype(v.dtype)
        if name != "iter":
            v[np.flatnonzero(rows)[0], 0] = np.nan          # Mandelbulb's linear plane legitimately holds NaN
        else:
            v[np.flatnonzero(rows)[0], 0] = -1


@pytest.mark.parametrize("f64", [False, True])
def test_sizes_patterns_and_alignment(f64):
    gp = _planes(f64)
    assert G.guard_elements(W) == 4096 and G.guard_elements(1000) == 8 * 1000 and G.guard_elements(1001) == 8 * 1008
    for name, p in gp.present():
        assert p.lo == G.guard_elements(W) * p.comps and p.total == p.n + 2 * p.lo
        assert (p.lo * p.dtype.itemsize) % 16 == 0
        assert p.bits().dtype.kind == "u" and np.all(p.bits() == p.pattern)
        assert p.payload().base is not None and p.payload().flags["C_CONTIGUOUS"]       # a view, not a copy
    assert gp["rgba"].address() % 16 == 0
    assert gp["nu"].dtype == (np.float64 if f64 else np.float32)
    assert np.isnan(gp["rgba"].values()).all() and np.isnan(gp["nu"].values()).all()      # quiet NaNs ...
    assert G.F32_PATTERN & 0x7FFFFF != 0x400000 and G.I32_PATTERN % 2 == 1                # ... with a payload; odd
    # before any store: everything unwritten, everything untouched
    assert gp.guards_intact() and gp.untouched(np.ones(ROWS, bool))
    assert gp.unwritten() == ROWS * W * 6 and gp.unwritten(MINE) == int(MINE.sum()) * W * 6


@pytest.mark.parametrize("f64", [False, True])
def test_a_correct_store_is_clean(f64):
    gp = _planes(f64)
    _store(gp)
    assert gp.guards_intact() and gp.unwritten() == 0 and gp.guard_hits() == {"rgba": 0, "nu": 0, "iter": 0}
    rgba, nu, it = gp.values()
    assert rgba.shape == (ROWS, W, 4) and nu.shape == (ROWS, W) and it.dtype == np.int32
    assert np.isnan(rgba[0, 0, 0]) and it[0, 0] == -1 and rgba[3, 2, 1] == np.float32((3 * W * 4 + 2 * 4 + 1) % 251)
    # a part of a whole-frame plane: its rows written, the others untouched
    gp = _planes(f64)
    _store(gp, MINE)
    assert gp.guards_intact() and gp.unwritten(MINE) == 0 and gp.untouched(~MINE)
    assert gp.unwritten() == int((~MINE).sum()) * W * 6


@pytest.mark.parametrize("name", G.GuardedPlanes.NAMES)
@pytest.mark.parametrize("f64", [False, True])
def test_each_wrong_store_is_reported(f64, name):
    def fresh():
        gp = _planes(f64)
        _store(gp, MINE)
        assert gp.guards_intact() and gp.unwritten(MINE) == 0 and gp.untouched(~MINE)
        return gp, gp[name]

    # one element past the end, one before the start: through a raw view of the buffer, as a kernel would
    for at in ("end", "start"):
        gp, p = fresh()
        raw = p._buf.view(p.dtype)
        raw[p.lo + p.n if at == "end" else p.lo - 1] = 0
        assert not p.guards_intact() and not gp.guards_intact() and gp.guard_hits()[name] == 1, at
        assert gp.unwritten(MINE) == 0 and gp.untouched(~MINE), at
    # the far ends of the bands are looked at too
    for k in (0, -1):
        gp, p = fresh()
        p._buf.view(p.dtype)[k] = 1
        assert not gp.guards_intact()
    # one payload element left alone
    gp, p = fresh()
    r = int(np.flatnonzero(MINE)[-1])
    p.payload_bits().reshape(ROWS, -1)[r, -1] = p.pattern
    assert gp.unwritten(MINE) == 1 and p.unwritten(MINE) == 1 and gp.unwritten() == int((~MINE).sum()) * W * 6 + 1
    assert gp.guards_intact() and gp.untouched(~MINE)
    # one element written in a foreign row, even a NaN or the value of its neighbour
    for value in (0, np.nan if name != "iter" else -1):
        gp, p = fresh()
        other = int(np.flatnonzero(~MINE)[0])
        p.payload(p.shape)[other, W - 1] = value
        assert not gp.untouched(~MINE) and not p.untouched(~MINE)
        assert gp.guards_intact() and gp.unwritten(MINE) == 0


def test_float_equality_is_never_used():
    """a kernel that stores the pattern's VALUE class (some other NaN) has written; one that stores nothing has not"""
    gp = _planes(False, planes=("nu",))
    v = gp["nu"].payload(gp["nu"].shape)
    v[:] = np.float32(np.nan)                                     # the default quiet NaN, not the pattern
    assert gp.unwritten() == 0
    gp["nu"].payload_bits()[5] = G.F32_PATTERN
    assert gp.unwritten() == 1


def test_absent_planes_and_the_raw_output():
    import ctypes
    import types

    class fr_output(ctypes.Structure):             # the C ABI's struct, restated: the checker's self-test needs no library
        _fields_ = [("rgba", ctypes.c_void_p), ("nu", ctypes.c_void_p), ("iter", ctypes.c_void_p), ("memory", ctypes.c_int32),
                    ("layout", ctypes.c_int32)]

    capi = types.SimpleNamespace(fr_output=fr_output, FR_MEM_DEVICE=0, FR_MEM_HOST=1, FR_LAYOUT_PACKED=0)
    gp = _planes(True, planes=("nu",))
    assert gp["rgba"] is None and gp["iter"] is None and gp.kwargs()["rgba"] is None
    assert [k for k, _ in gp.present()] == ["nu"]
    o = gp.output(capi, capi.FR_LAYOUT_PACKED)
    assert o.rgba is None and o.iter is None and o.nu == gp["nu"].address() and o.memory == capi.FR_MEM_HOST
    assert gp["nu"].address() == gp["nu"].payload().ctypes.data
    _store(gp)
    assert gp.guards_intact() and gp.unwritten() == 0 and gp.values()[0] is None
    with pytest.raises(AssertionError):
        _planes(True, planes=())


def test_byte_buffers_at_odd_offsets():
    """the export kernels' outputs: 1-D, any element type, the payload moved off the 4-byte boundary"""
    for dtype, pattern in ((np.uint8, 0xA5), (np.uint16, 0x5AA5)):
        for off in range(4):
            g = G.Guarded(61 * 3, dtype, pattern, 4096 + 16, "host", offset=off)
            assert g.address() % (4 * g.dtype.itemsize) == off * g.dtype.itemsize
            assert g.lo >= 4096 and g.total - g.lo - g.n >= 4096
            g.payload()[:] = 7
            assert g.guards_intact() and not g.still_pattern().any()
            g._buf[g.lo + g.n] = 7
            assert not g.guards_intact() and g.guard_hits() == 1
            g._buf[g.lo + g.n] = pattern
            g._buf[g.lo - 1] = 7
            assert not g.guards_intact()
            g._buf[g.lo - 1] = pattern
            g.payload()[17] = pattern
            assert g.guards_intact() and int(g.still_pattern().sum()) == 1
