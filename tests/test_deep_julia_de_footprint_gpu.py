"""The store footprint of the four deep_kernel<Julia, [X, ]DE[, BLA]> instantiations (fr_render_deep_julia_de and
fr_render_deepx_julia_de, plain and with their BLA flags): all five planes inside guard bands (tests/guarded.py), deriv at no more than a double's alignment, on a
frame whose edges are no sub-tile multiples and on one part of a 3-part sharding -- no byte outside a payload is touched, no
in-frame element stays unwritten, the rows of other parts stay as they were, and a plane that was not asked for is not written."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_julia_de_checks as K
import deep_julia_de_ref as JD
from test_deepx_de_footprint_gpu import Planes

pytestmark = pytest.mark.gpu

W, H = 21, 13
VIEW = {False: "DENDRITE30", True: "DENDRITE400"}      # the extended view starts extended and turns plain: both modes store
KERNELS = [(False, False), (False, True), (True, False), (True, True)]
IDS = ["DeepJuliaDeArgs", "DeepJuliaDeBlaArgs", "DeepJuliaXDeArgs", "DeepJuliaXDeBlaArgs"]     # the blocks' names at the time
EACH = pytest.mark.parametrize("ext,bla", KERNELS, ids=IDS)


@functools.lru_cache(maxsize=None)
def _reference(ext, bla):
    v = JD.view(VIEW[ext])
    (smp,), _ = K.restated(VIEW[ext], W, H, ext, 1, bla)
    return K.planes_of(v, smp, ext)


def _check(ext, bla, rows, P):
    it, de, deriv = _reference(ext, bla)
    if P.out is not None and P.out["iter"] is not None:
        assert np.array_equal(P.out["iter"].values((len(rows), W)), it[rows])
    if P.deriv is not None:
        assert np.array_equal(P.deriv.values(P.deriv.shape).view(np.uint64), np.ascontiguousarray(deriv[rows]).view(np.uint64))
    if P.de is not None:
        got, want = P.de.values(P.de.shape), de[rows]
        assert np.all(got[want == 0.0] == 0.0)
        nz = want != 0.0
        assert np.all(np.abs(got[nz] - want[nz]) <= K.DE_TOL * np.abs(want[nz]))


def _render(fr, renderer, ext, bla, P, shard=None):
    v = JD.view(VIEW[ext])
    renderer.render_deep_julia_de(K.state(fr, v), W, H, K.deep_view(fr, v, ext), bla=bla, shard=shard, **P.kwargs())


@EACH
@pytest.mark.parametrize("backend", ["device", "host"])
def test_whole_frame(fr, renderer, backend, ext, bla):
    P = Planes(H, W, backend)
    _render(fr, renderer, ext, bla, P)
    assert P.guards_intact(), [p.guard_hits() for p in P.all()]
    assert P.unwritten() == 0, [p.unwritten() for p in P.all()]
    _check(ext, bla, np.arange(H), P)


@EACH
@pytest.mark.parametrize("planes", [("de",), ("deriv",), ("iter", "deriv"), ("rgba", "de")], ids="+".join)
def test_planes_not_asked_for_are_not_written(fr, renderer, planes, ext, bla):
    P = Planes(H, W, "device", planes)
    bystanders = Planes(H, W, "device")
    _render(fr, renderer, ext, bla, P)
    assert P.guards_intact() and P.unwritten() == 0
    _check(ext, bla, np.arange(H), P)
    assert bystanders.guards_intact() and bystanders.untouched(np.ones(H, bool))


@EACH
def test_three_part_shard_in_frame_layout(fr, renderer, ext, bla):
    """part 1 of 3 alone into pattern-filled whole-frame planes, then the others"""
    E = fr._capi
    v = JD.view(VIEW[ext])
    P = Planes(H, W, "device")
    out = P.out.output(E, E.FR_LAYOUT_FRAME)
    e = E.fr_deep_de(P.de.address(), P.deriv.address(), 0, 1.8)
    p = K.state(fr, v).to_params(fr.FractalType.JuliaSet, fr.Precision.F64, False)
    if bla:
        p.flags |= fr.FR_FLAG_DEEPX_JULIA_BLA if ext else fr.FR_FLAG_DEEP_JULIA_BLA
    view = K.deep_view(fr, v, ext)
    cv = view.to_cx() if ext else view.to_c()
    entry = fr.lib().fr_render_deepx_julia_de if ext else fr.lib().fr_render_deep_julia_de
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
        P = Planes(len(g), W, backend)
        _render(fr, renderer, ext, bla, P, shard)
        assert P.guards_intact() and P.unwritten() == 0
        _check(ext, bla, g, P)
