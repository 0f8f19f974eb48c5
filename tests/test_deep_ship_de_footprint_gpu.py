"""The store footprint of the four deep_ship_de_kernel instantiations (fr_render_deep_ship_de and fr_render_deepx_ship_de, plain
and with their BLA flags): all five planes inside guard bands (tests/guarded.py), deriv four doubles per pixel at no more than a
double's alignment, on a frame whose edges are no sub-tile multiples and on one part of a 3-part sharding in FR_LAYOUT_FRAME -- no
byte outside a payload is touched, no in-frame element stays unwritten, the rows of other parts stay as they were, and a plane that
was not asked for is not written."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_ship_de_checks as K
from guarded import F64_PATTERN, Guarded, GuardedPlane, guard_elements
from test_deepx_de_footprint_gpu import Planes

pytestmark = pytest.mark.gpu

W, H = 21, 13
VIEW = {False: "A", True: "S310"}        # the extended view starts extended and turns plain: both modes store
KERNELS = [(False, False), (False, True), (True, False), (True, True)]
IDS = ["ShipDe", "ShipDeBla", "ShipXDe", "ShipXDeBla"]
EACH = pytest.mark.parametrize("ext,bla", KERNELS, ids=IDS)


class Deriv4Plane(GuardedPlane):
    """rows x W x 4 doubles whose payload starts 8 bytes off a 16-byte boundary: a caller's plane with a double's alignment"""

    def __init__(self, rows, W, backend):
        self.rows, self.W, self.comps = int(rows), int(W), 4
        Guarded.__init__(self, self.rows * self.W * 4, np.float64, F64_PATTERN, guard_elements(W) * 4, backend, offset=1)
        assert self.address() % 16 == 8


class ShipPlanes(Planes):
    """Planes with the ship's deriv: four doubles per pixel"""

    def __init__(self, rows, W, backend, planes=("rgba", "nu", "iter", "de", "deriv")):
        Planes.__init__(self, rows, W, backend, tuple(k for k in planes if k != "deriv"))
        self.deriv = Deriv4Plane(rows, W, backend) if "deriv" in planes else None


@functools.lru_cache(maxsize=None)
def _reference(ext, bla):
    v = K.view_of(VIEW[ext], ext)
    (smp,), _ = K.restated(VIEW[ext], W, H, ext, 1, bla)
    return K.planes_of(v, smp, ext)


def _check(ext, bla, rows, P):
    it, de, deriv = _reference(ext, bla)
    if P.out is not None and P.out["iter"] is not None:
        assert np.array_equal(P.out["iter"].values((len(rows), W)), it[rows])
    if P.deriv is not None:
        assert P.deriv.shape == (len(rows), W, 4)
        assert np.array_equal(P.deriv.values(P.deriv.shape).view(np.uint64), np.ascontiguousarray(deriv[rows]).view(np.uint64))
    if P.de is not None:
        got, want = P.de.values(P.de.shape), de[rows]
        assert np.all(got[want == 0.0] == 0.0)
        nz = want != 0.0
        assert np.all(np.abs(got[nz] - want[nz]) <= K.DE_TOL * np.abs(want[nz]))


def _render(fr, renderer, ext, bla, P, shard=None):
    v = K.view_of(VIEW[ext], ext)
    renderer.render_deep_ship_de(K.state(fr, v, ext), W, H, K.deep_view(fr, v, ext), bla=bla, shard=shard, **P.kwargs())


@EACH
@pytest.mark.parametrize("backend", ["device", "host"])
def test_whole_frame(fr, renderer, backend, ext, bla):
    P = ShipPlanes(H, W, backend)
    _render(fr, renderer, ext, bla, P)
    assert P.guards_intact(), [p.guard_hits() for p in P.all()]
    assert P.unwritten() == 0, [p.unwritten() for p in P.all()]
    _check(ext, bla, np.arange(H), P)
    it = _reference(ext, bla)[0]
    assert (it < K.view_of(VIEW[ext], ext)["max_iter"]).any()


@EACH
@pytest.mark.parametrize("planes", [("de",), ("deriv",), ("iter", "deriv"), ("rgba", "de")], ids="+".join)
def test_planes_not_asked_for_are_not_written(fr, renderer, planes, ext, bla):
    P = ShipPlanes(H, W, "device", planes)
    bystanders = ShipPlanes(H, W, "device")
    _render(fr, renderer, ext, bla, P)
    assert P.guards_intact() and P.unwritten() == 0
    _check(ext, bla, np.arange(H), P)
    assert bystanders.guards_intact() and bystanders.untouched(np.ones(H, bool))


@EACH
def test_three_part_shard_in_frame_layout(fr, renderer, ext, bla):
    """part 1 of 3 alone into pattern-filled whole-frame planes, the 4-double deriv plane among them, then the others"""
    E = fr._capi
    v = K.view_of(VIEW[ext], ext)
    P = ShipPlanes(H, W, "device")
    out = P.out.output(E, E.FR_LAYOUT_FRAME)
    e = E.fr_deep_de(P.de.address(), P.deriv.address(), 0, 1.8)
    p = K.state(fr, v, ext).to_params(fr.FractalType.BurningShip, fr.Precision.F64, False)
    if bla:
        p.flags |= E.FR_FLAG_DEEPX_SHIP_BLA if ext else E.FR_FLAG_DEEP_SHIP_BLA
    view = K.deep_view(fr, v, ext)
    cv = view.to_cx() if ext else view.to_c()
    entry = fr.lib().fr_render_deepx_ship_de if ext else fr.lib().fr_render_deep_ship_de
    for part in (1, 0, 2):
        shard = fr.Shard(part, 3, 2)
        g = shard.global_rows(H)
        sh = shard.to_c()
        assert entry(renderer._ctx, C.byref(p), C.byref(cv), C.byref(e), W, H, C.byref(sh), C.byref(out)) == E.FR_OK
        if part == 1:
            mine = np.zeros(H, bool)
            mine[g] = True
            assert mine.any() and not mine.all()
            assert P.guards_intact(), [q.guard_hits() for q in P.all()]
            assert P.unwritten(mine) == 0
            assert P.untouched(~mine)
    assert P.guards_intact(), [q.guard_hits() for q in P.all()]
    assert P.unwritten() == 0
    _check(ext, bla, np.arange(H), P)


@EACH
def test_packed_shard(fr, renderer, ext, bla):
    """one part's rows packed into planes of exactly its size, host and device"""
    shard = fr.Shard(1, 3, 2)
    g = shard.global_rows(H)
    for backend in ("device", "host"):
        P = ShipPlanes(len(g), W, backend)
        _render(fr, renderer, ext, bla, P, shard)
        assert P.guards_intact() and P.unwritten() == 0
        _check(ext, bla, g, P)
