"""Burning Ship zoom sequences on the GPU (fr_deep_ship_sequence_create): five frames at 64 x 48 over two octaves into the
centre of view S310 -- mode 0 against fr_render_deepx_ship byte for byte, mode 1 against the restated resampler
(tests/deep_seq_ref.py) applied to the GPU's own ship keyframes bit for bit, the keyframe reuse, plane requests, and the
two create calls each rejecting the other's fractal type."""
import ctypes as C

import numpy as np
import pytest

import deep_seq_ref as Q
import deepx_ship_ref as SX

pytestmark = pytest.mark.gpu

VIEW = SX.views()["S310"]
FIRST, LAST, N = "1e-310", "2.5e-311", 5
W, H = 64, 48


def _seq(fr, r, mode, **kw):
    return fr.DeepZoomSequence(r, fr.FractalState(max_iterations=VIEW["max_iter"]), VIEW["cx"], VIEW["cy"], FIRST, LAST, N, W, H,
                               keyframes=bool(mode), formula="ship", **kw)


def _planes(names=("rgba", "nu", "iter")):
    spec = dict(rgba=((H, W, 4), np.float32), nu=((H, W), np.float64), iter=((H, W), np.int32))
    return {k: np.full(spec[k][0], 77, spec[k][1]) for k in names}


def _frame(seq, f, names=("rgba", "nu", "iter")):
    p = _planes(names)
    seq.render(f, **p)
    return p


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_mode0_grid_frame_is_fr_render_deepx_ship(fr, renderer):
    with _seq(fr, renderer, 0) as seq:
        p = seq.plan(2)
        F = p.frac_bits
        assert F == Q.auto_frac_bits(FIRST, LAST) and not p.resampled and p.keyframe == 1
        got = _frame(seq, 2)
        want = _planes()
        renderer.render_deepx_ship(fr.FractalState(max_iterations=VIEW["max_iter"]), W, H,
                                   fr.DeepView(VIEW["cx"], VIEW["cy"], frac_bits=F, zoom="5e-311"), **want)
        for k in ("rgba", "nu", "iter"):
            assert _same(got[k], want[k]), k
        assert len(np.unique(want["iter"])) > 5 and np.all(want["rgba"][..., 3] == 1.0)
        # it is the ship: the Mandelbrot sequence of the same descriptor renders something else
        with fr.DeepZoomSequence(renderer, fr.FractalState(max_iterations=VIEW["max_iter"]), VIEW["cx"], VIEW["cy"], FIRST, LAST,
                                 N, W, H) as mseq:
            assert not _same(_frame(mseq, 2)["iter"], want["iter"])


def test_mode1_walk_resamples_the_ship_keyframes(fr):
    with fr.Renderer(0) as r:
        with _seq(fr, r, 1) as seq:
            one = [_frame(seq, f, ("rgba",))["rgba"] for f in range(N)]
            plans = [seq.plan(f) for f in range(N)]
            assert seq.stats() == (3, 2, 1)
            for names in (("nu",), ("iter",), ("rgba", "nu")):          # a resampled frame has an rgba plane only
                with pytest.raises(fr.FractalRendererError) as e:
                    _frame(seq, 1, names=names)
                assert e.value.status == fr._capi.FR_ERR_UNSUPPORTED
            assert seq.stats() == (3, 2, 1)
        with _seq(fr, r, 0) as s0:
            zero = [_frame(s0, f) for f in range(N)]
            assert s0.stats() == (5, 0, 0)                              # the same orbit key: the context still held it
    keys = {}
    for f in (0, 2, 4):
        assert not plans[f].resampled and plans[f].u == 1.0
        assert _same(one[f], zero[f]["rgba"]), f
        keys[plans[f].keyframe] = one[f]
    assert sorted(keys) == [0, 1, 2]
    for f in (1, 3):
        p = plans[f]
        assert p.resampled and 0.5 < p.u < 1.0
        want = Q.resample(keys[p.keyframe], keys[p.keyframe + 1], p.u)
        nbad = int((one[f].view(np.uint32) != want.view(np.uint32)).sum())
        print("frame", f, "float32 words that differ from the restated resampling", nbad)
        assert nbad == 0
        assert not _same(one[f], zero[f]["rgba"])                      # it IS resampled: not the exact render


def test_each_create_call_rejects_the_others_fractal(fr, renderer):
    L, K = fr.lib(), fr._capi
    d = K.fr_deep_sequence_desc(VIEW["cx"].encode(), VIEW["cy"].encode(), FIRST.encode(), LAST.encode(), N, 0, 1, 0)
    st = fr.FractalState(max_iterations=VIEW["max_iter"])
    ship = st.to_params(fr.FractalType.BurningShip, fr.Precision.F64, False)
    mand = st.to_params(fr.FractalType.Mandelbrot, fr.Precision.F64, False)
    h = C.c_void_p()
    assert L.fr_deep_sequence_create(renderer._ctx, C.byref(ship), C.byref(d), W, H, C.byref(h)) == K.FR_ERR_UNSUPPORTED
    assert not h.value
    assert L.fr_deep_ship_sequence_create(renderer._ctx, C.byref(mand), C.byref(d), W, H, C.byref(h)) == K.FR_ERR_UNSUPPORTED
    assert not h.value
    bad = K.fr_deep_sequence_desc(VIEW["cx"].encode(), VIEW["cy"].encode(), FIRST.encode(), LAST.encode(), N, 0, 1, 1)
    assert L.fr_deep_ship_sequence_create(renderer._ctx, C.byref(ship), C.byref(bad), W, H, C.byref(h)) == K.FR_ERR_INVALID_ARG
    flagged = st.to_params(fr.FractalType.BurningShip, fr.Precision.F64, False)
    flagged.flags |= K.FR_FLAG_DEEPX_BLA
    assert L.fr_deep_ship_sequence_create(renderer._ctx, C.byref(flagged), C.byref(d), W, H, C.byref(h)) == K.FR_ERR_UNSUPPORTED
    assert L.fr_deep_ship_sequence_create(renderer._ctx, C.byref(ship), C.byref(d), W, H, C.byref(h)) == K.FR_OK and h.value
    L.fr_deep_sequence_destroy(h)
