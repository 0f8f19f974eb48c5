"""The cache slot of a deep path, reused: every one of the six paths (fp64 and extended storage; Mandelbrot, Burning Ship,
Julia), without and with its BLA flag, renders view A, then a view B with a shorter orbit and a smaller max_iter -- the slot
shrinks in use, not in capacity, and the upload covers what the host wrote and nothing else -- then A again on a second stream
without waiting.  Every render equals the render of its view on a context that has seen nothing else, byte for byte, and the
table builds are counted as they always were: one per new orbit, none without the flag, none for a Julia zoom change."""
import numpy as np
import pytest

import deep_cases as DC
import deep_julia_ref as J
import deep_ref as R
import deep_ship_ref as S

pytestmark = pytest.mark.gpu

W, H = 32, 24

# path -> (extended storage, formula as fr_deep_bla_builds numbers it, view A, view B); every max_iter <= 300
_JA = dict(J.view("DENDRITE30"), max_iter=256, frac_bits=256)      # F given: the automatic one follows the zoom
_JB = dict(J.view("BASILICA30"), max_iter=64, frac_bits=256)
PATHS = {
    "deep": (0, 0, R.VIEW_A, DC.SMALL_M),
    "deepx": (1, 0, R.VIEW_A, DC.SMALL_M),
    "deep_ship": (0, 1, S.SHIP_A, DC.SMALL_S),
    "deepx_ship": (1, 1, S.SHIP_A, DC.SMALL_S),
    "deep_julia": (0, 2, _JA, _JB),
    "deepx_julia": (1, 2, _JA, _JB),
}


def _render(fr, r, path, v, bla, planes=None, **kw):
    """one 32 x 24 frame of v through the path's entry point; planes: (rgba, nu, iter), host arrays of its own by default"""
    ext, formula = PATHS[path][:2]
    rgba, nu, it = planes or (np.empty((H, W, 4), np.float32), np.empty((H, W), np.float64), np.empty((H, W), np.int32))
    c = v.get("c", (0.0, 0.0))
    st = fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"], julia_c_real=c[0], julia_c_imag=c[1])
    view = fr.DeepView(v["cx"], v["cy"], v.get("frac_bits", 0), zoom=repr(v["zoom"]) if ext else None)
    out = dict(rgba=rgba, nu=nu, iter=it, **kw)
    if formula == 0:
        r.render_deep(st, W, H, view, **out, **({"xbla": bla} if ext else {"bla": bla}))
    elif formula == 1:
        (r.render_deepx_ship if ext else r.render_deep_ship)(st, W, H, view, bla=bla, **out)
    else:
        r.render_deep_julia(st, W, H, view, bla=bla, **out)
    return rgba, nu, it


def _orbit_lengths(fr, formula, v):
    """points of the view's reference orbit(s) as the host computes them (the same in either storage)"""
    view = fr.DeepView(v["cx"], v["cy"], v.get("frac_bits", 0))
    if formula == 2:
        return [len(o) for o in fr.deep_julia_reference_orbits(view, v["c"], v["max_iter"], zoom=v["zoom"])]
    return [len((fr.deep_ship_reference_orbit if formula == 1 else fr.deep_reference_orbit)(view, v["zoom"], v["max_iter"]))]


def _same(got, want):
    return all(np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)) for g, w in zip(got, want))


@pytest.mark.parametrize("bla", [False, True], ids=["plain", "bla"])
@pytest.mark.parametrize("path", list(PATHS))
def test_a_shrunk_slot_renders_the_first_view_again(fr, path, bla):
    import torch
    ext, formula, A, B = PATHS[path]
    assert B["max_iter"] < A["max_iter"] <= 300
    assert max(_orbit_lengths(fr, formula, B)) < min(_orbit_lengths(fr, formula, A))   # every orbit of B ends inside A's
    L = fr.lib()
    with fr.Renderer(0) as r:
        alone = _render(fr, r, path, A, bla)
    with fr.Renderer(0) as r:
        other_alone = _render(fr, r, path, B, bla)
    with fr.Renderer(0) as r:
        builds = lambda: int(L.fr_deep_bla_builds(r._ctx, ext, formula))
        assert builds() == 0
        first = _render(fr, r, path, A, bla)
        assert builds() == (1 if bla else 0)
        other = _render(fr, r, path, B, bla)
        assert builds() == (2 if bla else 0)
        assert not np.array_equal(other[2], first[2])
        dev = torch.device("cuda:0")
        planes = (torch.zeros((H, W, 4), dtype=torch.float32, device=dev), torch.zeros((H, W), dtype=torch.float64, device=dev),
                  torch.full((H, W), -7, dtype=torch.int32, device=dev))
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        _render(fr, r, path, A, bla, planes, stream=s.cuda_stream, sync=False)
        s.synchronize()
        r.check()
        again = tuple(t.cpu().numpy() for t in planes)
        assert builds() == (3 if bla else 0)
        if formula == 2:                                          # Julia: the tables do not depend on the zoom
            _render(fr, r, path, dict(A, zoom=2e-30), bla)
            assert builds() == (3 if bla else 0)
    assert _same(first, alone), path
    assert _same(other, other_alone), path                        # B behind A's longer orbits: nothing past B's own is read
    assert _same(again, alone), path
