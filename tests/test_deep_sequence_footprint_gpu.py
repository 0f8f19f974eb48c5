"""The store footprint of deep zoom sequences (fr_deep_sequence): guard-banded planes (tests/guarded.py) around a resampled
frame of the standard sequence S (deep_resample_kernel) at sizes from one pixel to several blocks of odd width -- (a) no
byte outside the plane is touched, (b) no pixel stays unwritten, alpha is 1, (c) what is written equals the restated
resampling (tests/deep_seq_ref.py) of the sequence's own keyframes -- and around an exact mode-0 frame."""
import numpy as np
import pytest

import deep_seq_ref as Q
import deepx_ref as X
from guarded import GuardedPlanes

pytestmark = pytest.mark.gpu

T110 = X.views()["T110"]
S = Q.S
SIZES = [(1, 1), (7, 5), (64, 48), (203, 117)]


def _seq(fr, r, mode, W, H):
    return fr.DeepZoomSequence(r, fr.FractalState(max_iterations=S["max_iter"]), T110["cx"], T110["cy"], S["zoom_first"],
                               S["zoom_last"], S["frames"], W, H, keyframes=bool(mode))


@pytest.mark.parametrize("backend", ["device", "host"])
@pytest.mark.parametrize("geom", SIZES, ids=lambda g: "%dx%d" % g)
def test_resampled_frame(fr, renderer, geom, backend):
    W, H = geom
    with _seq(fr, renderer, 1, W, H) as seq:
        p = seq.plan(2)
        assert p.resampled and p.keyframe == 0
        gp = GuardedPlanes(H, W, f64=True, backend=backend, planes=("rgba",))
        seq.render(2, **gp.kwargs())
        assert gp.guards_intact(), gp.guard_hits()
        assert gp.unwritten() == 0
        rgba, _, _ = gp.values()
        assert np.all(rgba[..., 3] == 1.0)
        keys = []
        for f in (0, 4):                                               # keyframes 0 and 1, as the sequence holds them
            k = np.empty((H, W, 4), np.float32)
            seq.render(f, rgba=k)
            keys.append(k)
        assert seq.stats()[:2] == (2, 1)                               # the two keyframes were rendered once, for frame 2
        want = Q.resample(keys[0], keys[1], p.u)
        assert np.array_equal(rgba.view(np.uint32), want.view(np.uint32)), int((rgba.view(np.uint32) != want.view(np.uint32)).sum())


@pytest.mark.parametrize("backend", ["device", "host"])
def test_exact_frame(fr, renderer, backend):
    W, H = 7, 5
    with _seq(fr, renderer, 0, W, H) as seq:
        gp = GuardedPlanes(H, W, f64=True, backend=backend)
        seq.render(2, **gp.kwargs())
        assert gp.guards_intact(), gp.guard_hits()
        assert gp.unwritten() == 0, {k: q.unwritten() for k, q in gp.present()}
        rgba, nu, it = gp.values()
        assert np.all(rgba[..., 3] == 1.0)
        plain = dict(rgba=np.empty((H, W, 4), np.float32), nu=np.empty((H, W)), iter=np.empty((H, W), np.int32))
        seq.render(2, **plain)
        assert np.array_equal(rgba.view(np.uint32), plain["rgba"].view(np.uint32))
        assert np.array_equal(nu.view(np.uint64), plain["nu"].view(np.uint64)) and np.array_equal(it, plain["iter"])
