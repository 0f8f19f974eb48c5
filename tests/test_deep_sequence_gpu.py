"""Deep zoom sequences on the GPU (fr_deep_sequence): mode 0 against fr_render_deepx (grid frames, byte for byte) and the
numpy restatement of the two-mode step (off-grid frames, the extended range), mode 1 against the restated resampler
(tests/deep_seq_ref.py) applied to the GPU's own keyframes, bit for bit; the one orbit, the keyframe reuse, plane
requests, zoom-out, the quality condition that makes reuse worth having, and the PNG forms."""
import functools
import os

import numpy as np
import pytest

import deep_ref as R
import deep_seq_ref as Q
import deepx_ref as X

pytestmark = pytest.mark.gpu

V = X.views()
S = Q.S
T110 = V["T110"]
W, H = 64, 48
N = S["frames"]
GRID = Q.S_GRID


def _seq(fr, r, mode, w=W, h=H, first=S["zoom_first"], last=S["zoom_last"], frames=N, view=T110, max_iter=S["max_iter"], **kw):
    return fr.DeepZoomSequence(r, fr.FractalState(max_iterations=max_iter), view["cx"], view["cy"], first, last, frames, w, h,
                               keyframes=bool(mode), **kw)


def _host_planes(w=W, h=H, names=("rgba", "nu", "iter")):
    spec = dict(rgba=((h, w, 4), np.float32), nu=((h, w), np.float64), iter=((h, w), np.int32))
    return {k: np.full(spec[k][0], 77, spec[k][1]) for k in names}


def _frame(seq, f, w=W, h=H, names=("rgba", "nu", "iter")):
    p = _host_planes(w, h, names)
    seq.render(f, **p)
    return p


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _deepx(fr, r, zoom, F, w=W, h=H, **kw):
    p = _host_planes(w, h)
    r.render_deep(fr.FractalState(max_iterations=S["max_iter"]), w, h,
                  fr.DeepView(T110["cx"], T110["cy"], frac_bits=F, zoom=zoom), **p, **kw)
    return p


@functools.lru_cache(maxsize=None)
def _walks(fr, w, h, post):
    """On a context of its own: the mode-1 walk over S (frames in order), its stats, then every frame in mode 0"""
    with fr.Renderer(0) as r:
        with _seq(fr, r, 1, w, h, post_chain=post) as s1:
            one = [_frame(s1, f, w, h, ("rgba",))["rgba"] for f in range(N)]
            stats1 = s1.stats()
            plans = [s1.plan(f) for f in range(N)]
        with _seq(fr, r, 0, w, h, post_chain=post) as s0:
            zero = [_frame(s0, f, w, h) for f in range(N)]
            stats0 = s0.stats()
    return dict(one=one, zero=zero, stats1=stats1, stats0=stats0, plans=plans)


# 1. mode 0, frames on the grid: fr_render_deepx with the decimal string and frac_bits = F
@pytest.mark.parametrize("xbla", [False, True])
def test_mode0_grid_frames_are_fr_render_deepx(fr, renderer, xbla):
    import torch
    with _seq(fr, renderer, 0, xbla=xbla) as seq:
        F = seq.plan(0).frac_bits
        assert F == Q.auto_frac_bits(S["zoom_first"], S["zoom_last"])
        for f, zoom in GRID.items():
            want = _deepx(fr, renderer, zoom, F, xbla=xbla)
            got = _frame(seq, f)
            dev = dict(rgba=torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0"),
                       nu=torch.zeros((H, W), dtype=torch.float64, device="cuda:0"),
                       iter=torch.zeros((H, W), dtype=torch.int32, device="cuda:0"))
            torch.cuda.synchronize()
            seq.render(f, **dev)
            for k in ("rgba", "nu", "iter"):
                assert _same(got[k], want[k]), (f, k)
                assert _same(dev[k].cpu().numpy(), want[k]), (f, k, "device")
            assert len(np.unique(want["iter"])) > 5 and np.all(want["rgba"][..., 3] == 1.0)


def _restated_frame(view, first, last, frames, f, w, h):
    p = Q.plan(first, last, frames, f)
    F = Q.auto_frac_bits(first, last)
    mant, exp2 = X.reference_orbit_x(view["cx"], view["cy"], F, view["max_iter"])
    stats = {}
    it, r2 = X.perturb_x(mant, exp2, X.sample_dc_x(w, h, p["zoom_mant"], p["zoom_exp2"], 1, 0), view["max_iter"], stats=stats)
    return it.reshape(h, w), r2.reshape(h, w), stats, p


def _check_restated(seq, view, first, last, frames, f, w, h):
    it, r2, stats, want = _restated_frame(view, first, last, frames, f, w, h)
    p = seq.plan(f)
    assert (p.zoom_mant, p.zoom_exp2) == (want["zoom_mant"], want["zoom_exp2"]) and not p.resampled
    got = _frame(seq, f, w, h)
    ndiff = int((got["iter"] != it).sum())
    dnu = float(np.abs(got["nu"] - R.smooth(it, r2, view["max_iter"])).max())
    print("frame", f, "iter differences", ndiff, "max |nu - restated|", dnu, stats)
    assert ndiff == 0 and dnu <= 1e-9
    assert len(np.unique(it)) > 5 and np.all(got["rgba"][..., 3] == 1.0)
    return stats


# 2. mode 0, a frame off the grid: the restatement at the planned pair
def test_mode0_off_grid_frame_matches_the_restatement(fr, renderer):
    with _seq(fr, renderer, 0) as seq:
        _check_restated(seq, T110, S["zoom_first"], S["zoom_last"], N, 2, W, H)


# 3. mode 0 in the extended range: the deltas are extended numbers for a long stretch of every sample's orbit
def test_mode0_in_the_extended_range(fr, renderer):
    v = V["T300"]
    w, h = 16, 12
    with _seq(fr, renderer, 0, w, h, "1e-300", "2.5e-301", 5, view=v, max_iter=v["max_iter"]) as seq:
        stats = _check_restated(seq, v, "1e-300", "2.5e-301", 5, 1, w, h)
        assert stats["ext_steps"] > 10 * w * h and stats["to_plain"] > 0


# 4. / 5. the walks: one orbit, each keyframe once
def test_mode0_walk_computes_one_orbit(fr):
    with fr.Renderer(0) as r, _seq(fr, r, 0) as seq:
        for f in range(N):
            _frame(seq, f, names=("rgba",))
        assert seq.stats() == (9, 0, 1)


@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("w,h", [(W, H), (203, 117)])
def test_mode1_walk(fr, w, h, post):
    wk = _walks(fr, w, h, post)
    assert wk["stats1"] == (3, 6, 1)
    assert wk["stats0"] == (9, 0, 0)                                   # the same orbit key: the context still held it
    keys = {}
    for f in GRID:
        assert _same(wk["one"][f], wk["zero"][f]["rgba"]), f
        p = wk["plans"][f]
        assert not p.resampled and p.u == 1.0
        keys[p.keyframe] = wk["one"][f]
    for f in range(N):
        if f in GRID:
            continue
        p = wk["plans"][f]
        assert p.resampled and 0.5 < p.u < 1.0
        want = Q.resample(keys[p.keyframe], keys[p.keyframe + 1], p.u)
        got = wk["one"][f]
        nbad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        print(w, h, post, "frame", f, "float32 words that differ from the restated resampling", nbad)
        assert nbad == 0
        assert not _same(got, wk["zero"][f]["rgba"])                   # it IS resampled: not the exact render
    # the two kinds of colour are different planes: the post chain went through the keyframes
    assert not _same(wk["one"][1], _walks(fr, w, h, not post)["one"][1])


# 6. any order
def test_mode1_out_of_order(fr, renderer):
    wk = _walks(fr, W, H, False)
    with _seq(fr, renderer, 1) as seq:
        for f in (6, 1, 8, 3):
            assert _same(_frame(seq, f, names=("rgba",))["rgba"], wk["one"][f]), f
        exact, resampled, _ = seq.stats()
        assert resampled == 3 and exact >= 3


# 7. which planes a frame has
def test_mode1_plane_requests(fr, renderer):
    wk = _walks(fr, W, H, False)
    with _seq(fr, renderer, 1) as seq:
        for names in (("nu",), ("iter",), ("rgba", "nu"), ("rgba", "nu", "iter")):
            with pytest.raises(fr.FractalRendererError) as e:
                _frame(seq, 2, names=names)
            assert e.value.status == fr._capi.FR_ERR_UNSUPPORTED
        assert seq.stats()[:2] == (0, 0)
        for f in (4, 0, 4):                                            # the second visit of 4 finds its keyframe cached
            got = _frame(seq, f)
            for k in ("rgba", "nu", "iter"):
                assert _same(got[k], wk["zero"][f][k]), (f, k)
        got = _frame(seq, 8, names=("nu", "iter"))
        assert _same(got["nu"], wk["zero"][8]["nu"]) and _same(got["iter"], wk["zero"][8]["iter"])
        assert _same(_frame(seq, 6, names=("rgba",))["rgba"], wk["one"][6])
        with pytest.raises(fr.FractalRendererError):
            _frame(seq, N)


# 8. zoom-out
def test_mode1_zoom_out_mirrors_the_zoom_in(fr, renderer):
    wk = _walks(fr, W, H, False)
    with _seq(fr, renderer, 1, first=S["zoom_last"], last=S["zoom_first"]) as seq:
        for f in range(N):
            assert seq.plan(f).keyframe <= 0
            assert _same(_frame(seq, f, names=("rgba",))["rgba"], wk["one"][N - 1 - f]), f
        assert seq.stats()[:2] == (3, 6)


# 9. reuse is worth having: a resampled frame is far closer to the exact one than either keyframe shown in its place
@pytest.mark.parametrize("post", [False, True])
def test_resampled_frames_beat_their_unresampled_keyframes(fr, post):
    wk = _walks(fr, W, H, post)
    for f in (1, 2, 3):
        exact = wk["zero"][f]["rgba"].astype(np.float64)
        err = np.abs(wk["one"][f] - exact).mean()
        shown = min(np.abs(wk["zero"][k]["rgba"] - exact).mean() for k in (0, 4))
        print("post", post, "frame", f, "mean |mode 1 - mode 0|", err, "nearest keyframe unresampled", shown, "ratio", err / shown)
        assert err < 0.5 * shown


# 10. the PNG forms
def test_render_png_and_render_to_folder(fr, renderer, tmp_path):
    from pngdec import read_png
    for mode in (1, 0):
        with _seq(fr, renderer, mode, post_chain=True) as seq:
            for f in (0, 2):
                rgba = _frame(seq, f, names=("rgba",))["rgba"]
                want = renderer.export_rgb8(rgba, W, H, through_half=True)
                path = str(tmp_path / f"m{mode}_{f}.png")
                seq.render_png(f, path)
                px, _ = read_png(path)
                assert px.shape == (H, W, 3) and np.array_equal(px, want), (mode, f)
    with _seq(fr, renderer, 1) as seq:                                  # created without the post chain: the PNG has it all the same
        path = str(tmp_path / "linear.png")
        seq.render_png(2, path)
        assert np.array_equal(read_png(path)[0], read_png(str(tmp_path / "m1_2.png"))[0])
        folder = str(tmp_path / "all")
        seen = []
        assert seq.render_to_folder(folder, lambda f, n: seen.append((f, n))) == N
        assert sorted(os.listdir(folder)) == [os.path.basename(fr.frame_path(folder, f)) for f in range(N)]
        assert seen == [(f, N) for f in range(N)]
        assert np.array_equal(read_png(fr.frame_path(folder, 2))[0], read_png(path)[0])
        part = str(tmp_path / "part")
        assert seq.render_to_folder(part, lambda f, n: f == 2) == 3
        assert sorted(os.listdir(part)) == [os.path.basename(fr.frame_path(part, f)) for f in range(3)]
