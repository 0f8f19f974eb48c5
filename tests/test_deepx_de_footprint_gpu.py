"""The store footprint of deep_kernel<Mandel, X, DE> and deep_kernel<Mandel, X, DE, BLA> (fr_render_deepx_de, plain and
with FR_FLAG_DEEPX_BLA): all five planes inside guard bands (tests/guarded.py), deriv at no more than a double's alignment, on
frames whose edges are no sub-tile multiples and on one part of a 3-part sharding written in place -- no byte outside a payload
is touched, no in-frame element stays unwritten, the rows of other parts stay as they were, and a plane that was not asked for
is not written."""
import ctypes as C
import functools

import numpy as np
import pytest

import deepx_de_ref as XD
import deepx_ref as X
from guarded import F64_PATTERN, Guarded, GuardedPlane, GuardedPlanes, guard_elements

pytestmark = pytest.mark.gpu

VIEW = X.views()["T130"]               # starts extended and turns plain: both modes store through the same epilogue
SIZES = [(1, 1), (7, 5), (21, 13), (67, 37)]
KERNELS = ["plain", "bla"]


@functools.lru_cache(maxsize=None)
def _orbit():
    return X.orbit_of(VIEW)


@functools.lru_cache(maxsize=None)
def _reference(W, H, bla):
    (smp,), _ = XD.restate_x_de(VIEW, W, H, bla=bla, orbit=_orbit())
    it, r2, Dx, Dy, eD = smp
    return it, XD.deriv_of_x(it, Dx, Dy, eD, VIEW["max_iter"]), XD.de_of_x(it, r2, Dx, Dy, eD, VIEW["max_iter"])


def _state(fr):
    return fr.FractalState(max_iterations=VIEW["max_iter"])


def _view(fr):
    return fr.DeepView(VIEW["cx"], VIEW["cy"], zoom=VIEW["zoom"])


class DerivPlane(GuardedPlane):
    """rows x W x 2 doubles whose payload starts 8 bytes off a 16-byte boundary: a caller's plane with a double's alignment"""

    def __init__(self, rows, W, backend):
        self.rows, self.W, self.comps = int(rows), int(W), 2
        Guarded.__init__(self, self.rows * self.W * 2, np.float64, F64_PATTERN, guard_elements(W) * 2, backend, offset=1)
        assert self.address() % 16 == 8


class Planes:
    """GuardedPlanes with the two planes of fr_deep_de"""

    def __init__(self, rows, W, backend, planes=("rgba", "nu", "iter", "de", "deriv")):
        three = tuple(k for k in planes if k in GuardedPlanes.NAMES)
        self.out = GuardedPlanes(rows, W, f64=True, backend=backend, planes=three) if three else None
        self.de = GuardedPlane(rows, W, 1, np.float64, F64_PATTERN, backend) if "de" in planes else None
        self.deriv = DerivPlane(rows, W, backend) if "deriv" in planes else None

    def all(self):
        return ([p for _, p in self.out.present()] if self.out else []) + [p for p in (self.de, self.deriv) if p is not None]

    def kwargs(self):
        kw = self.out.kwargs() if self.out else {}
        kw.update(de=None if self.de is None else self.de.payload(self.de.shape),
                  deriv=None if self.deriv is None else self.deriv.payload(self.deriv.shape))
        return kw

    def guards_intact(self):
        return all(p.guards_intact() for p in self.all())

    def unwritten(self, rows_mask=None):
        return sum(p.unwritten(rows_mask) for p in self.all())

    def untouched(self, rows_mask):
        return all(p.untouched(rows_mask) for p in self.all())


def _check(W, H, bla, rows, P):
    it, deriv, de = _reference(W, H, bla)
    if P.out is not None and P.out["iter"] is not None:
        assert np.array_equal(P.out["iter"].values((len(rows), W)), it[rows])
    if P.deriv is not None:
        assert np.array_equal(P.deriv.values(P.deriv.shape).view(np.uint64), np.ascontiguousarray(deriv[rows]).view(np.uint64))
    if P.de is not None:
        got, want = P.de.values(P.de.shape), de[rows]
        assert np.all(got[want == 0.0] == 0.0)
        nz = want != 0.0
        assert np.all(np.abs(got[nz] - want[nz]) <= 2.0 ** -50 * np.abs(want[nz]))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("backend", ["device", "host"])
@pytest.mark.parametrize("geom", SIZES, ids=lambda g: "%dx%d" % g)
def test_whole_frame(fr, renderer, geom, backend, kernel):
    W, H = geom
    P = Planes(H, W, backend)
    renderer.render_deepx_de(_state(fr), W, H, _view(fr), bla=kernel == "bla", **P.kwargs())
    assert P.guards_intact(), [p.guard_hits() for p in P.all()]
    assert P.unwritten() == 0, [p.unwritten() for p in P.all()]
    _check(W, H, kernel == "bla", np.arange(H), P)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("planes", [("de",), ("deriv",), ("iter", "deriv"), ("rgba", "de")], ids="+".join)
def test_planes_not_asked_for_are_not_written(fr, renderer, planes, kernel):
    """the ragged frame with a subset of the planes: those are complete, and guarded planes the call never got stay pattern"""
    W, H = 21, 13
    P = Planes(H, W, "device", planes)
    bystanders = Planes(H, W, "device")
    renderer.render_deepx_de(_state(fr), W, H, _view(fr), bla=kernel == "bla", **P.kwargs())
    assert P.guards_intact() and P.unwritten() == 0
    _check(W, H, kernel == "bla", np.arange(H), P)
    assert bystanders.guards_intact() and bystanders.untouched(np.ones(H, bool))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("geom", SIZES[1:], ids=lambda g: "%dx%d" % g)
def test_three_part_shard_in_frame_layout(fr, renderer, geom, kernel):
    """part 1 of 3 alone into pattern-filled whole-frame planes, then the others"""
    W, H = geom
    E = fr._capi
    P = Planes(H, W, "device")
    out = P.out.output(E, E.FR_LAYOUT_FRAME)
    e = E.fr_deep_de(P.de.address(), P.deriv.address(), 0, 1.8)
    p = _state(fr).to_params(fr.FractalType.Mandelbrot, fr.Precision.F64, False)
    if kernel == "bla":
        p.flags |= fr.FR_FLAG_DEEPX_BLA
    cv = _view(fr).to_cx()
    strip = 2 if H < 16 else 8
    for part in (1, 0, 2):
        shard = fr.Shard(part, 3, strip)
        g = shard.global_rows(H)
        sh = shard.to_c()
        assert fr.lib().fr_render_deepx_de(renderer._ctx, C.byref(p), C.byref(cv), C.byref(e), W, H, C.byref(sh), C.byref(out)) == E.FR_OK
        if part == 1:
            mine = np.zeros(H, bool)
            mine[g] = True
            assert mine.any() and not mine.all()
            assert P.guards_intact(), [q.guard_hits() for q in P.all()]
            assert P.unwritten(mine) == 0
            assert P.untouched(~mine)
    assert P.guards_intact(), [q.guard_hits() for q in P.all()]
    assert P.unwritten() == 0
    _check(W, H, kernel == "bla", np.arange(H), P)


@pytest.mark.parametrize("kernel", KERNELS)
def test_packed_shard(fr, renderer, kernel):
    """one part's rows packed into planes of exactly its size, host and device"""
    W, H = 21, 13
    shard = fr.Shard(1, 3, 2)
    g = shard.global_rows(H)
    for backend in ("device", "host"):
        P = Planes(len(g), W, backend)
        renderer.render_deepx_de(_state(fr), W, H, _view(fr), bla=kernel == "bla", shard=shard, **P.kwargs())
        assert P.guards_intact() and P.unwritten() == 0
        _check(W, H, kernel == "bla", g, P)
