"""The folded render's decision and its division helper, without a GPU.

A Mandelbrot frame with center_y == 0 is symmetric about the real axis bit for bit, so it renders its first
R = floor(H / 2) + 1 rows (rounded up to whole 8-row sub-tile rows) and stores every finished pixel of row r at row H - r
too (fr_plan.h: plan_fold; option "fold").  fr_fold_describe answers for a request what enqueue_render decides; the matrix
below has the qualifying case and every condition switched off on its own.  fr_fold_division hands out the multiplier and
shift with which the lane pool finds the row of a plane index; the checks evaluate the kernel's expression
(index * magic) >> shift in Python's integers.
"""
import pytest

BIG = (1024, 1024)          # 2^20 pixels: the smallest frame the automatic setting folds


def _params(K, **kw):
    p = K.fr_params()
    K.check(K.lib().fr_params_default(p))
    p.fractal_type, p.precision, p.max_iterations = 0, 1, 256
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _fold(fr, W, H, shard=None, tunings=(), **kw):
    K = fr._capi
    return K.fold_describe(_params(K, **kw), W, H, K.fr_shard(*shard) if shard else None, tunings)


def _R(H):
    return (H // 2 + 1 + 7) // 8 * 8


def test_default_view_qualifies(fr):
    K = fr._capi
    p = _params(K)
    assert p.center_y == 0.0, "the default view lies on the real axis"
    assert _fold(fr, *BIG) == {"fold": True, "rows_rendered": _R(1024)}
    assert _fold(fr, *BIG, tunings=(("fold", 2),)) == {"fold": True, "rows_rendered": 520}
    assert _fold(fr, 257, 130, tunings=(("fold", 2),)) == {"fold": True, "rows_rendered": 72}
    assert _fold(fr, *BIG, precision=0) == {"fold": True, "rows_rendered": 520}


@pytest.mark.parametrize("name,kw,shard,W,H,tunings", [
    ("center_y 0.1", dict(center_y=0.1), None, *BIG, ()),
    ("center_y 1e-300 in fp64", dict(center_y=1e-300), None, *BIG, ()),
    ("Julia", dict(fractal_type=1), None, *BIG, ()),
    ("Burning Ship", dict(fractal_type=2), None, *BIG, ()),
    ("stripe", dict(stripe_enabled=1), None, *BIG, ()),
    ("trap", dict(orbit_trap_enabled=1), None, *BIG, ()),
    ("interior style 2", dict(interior_style=2), None, *BIG, ()),
    ("aa 2", dict(antialiasing_samples=2), None, *BIG, ()),
    ("2-part shard", {}, (0, 2, 8), *BIG, ()),
    ("Deep_Zoom", dict(fractal_type=5), None, *BIG, ()),
    ("R >= H", {}, None, 64, 16, (("fold", 2),)),
    ("below 2^20 pixels, automatic", {}, None, 1024, 1023, ()),
    ("fold = 1", {}, None, *BIG, (("fold", 1),)),
    ("general tile kernel", {}, None, *BIG, (("tile_kernel", 1),)),
    ("16x4 sub-tiles", {}, None, *BIG, (("subtile_shape", 4),)),
])
def test_each_condition_alone_switches_it_off(fr, name, kw, shard, W, H, tunings):
    for t in (tunings, tuple(tunings) + ((("fold", 2),) if not any(k == "fold" for k, _ in tunings) and "automatic" not in name else ())):
        got = _fold(fr, W, H, shard, t, **kw)
        assert got["fold"] is False, (name, t)
        rows = H if not shard else fr.Shard(*shard).rows(H)
        assert got["rows_rendered"] == rows, (name, t)
    # ... and the same request without that condition folds
    if "automatic" not in name and name != "R >= H":
        assert _fold(fr, *BIG, tunings=(("fold", 2),))["fold"] is True


def test_below_the_automatic_size_fold_2_still_folds(fr):
    assert _fold(fr, 1024, 1023) == {"fold": False, "rows_rendered": 1023}
    assert _fold(fr, 1024, 1023, tunings=(("fold", 2),)) == {"fold": True, "rows_rendered": 512}


def test_negative_zero_and_values_that_cast_to_zero(fr):
    assert _fold(fr, *BIG, center_y=-0.0)["fold"] is True
    assert _fold(fr, *BIG, center_y=-0.0, precision=0)["fold"] is True
    assert _fold(fr, *BIG, center_y=1e-60, precision=0)["fold"] is True, "1e-60 is 0 in the fp32 kernels"
    assert _fold(fr, *BIG, center_y=1e-60, precision=1)["fold"] is False
    assert _fold(fr, *BIG, center_y=float("nan"))["fold"] is False


@pytest.mark.parametrize("H,R", [(16, 16), (17, 16), (129, 72), (130, 72), (4096, 2056), (24, 16), (190, 96)])
def test_rows_rendered(fr, H, R):
    assert _R(H) == R
    got = _fold(fr, 64, H, tunings=(("fold", 2),))
    assert got == ({"fold": True, "rows_rendered": R} if R < H else {"fold": False, "rows_rendered": H})
    if got["fold"]:
        # every row is rendered or is the mirror of exactly one rendered row: targets H - r for r in [1, R) with H - r >= R
        targets = [H - r for r in range(1, R) if H - r >= R]
        assert sorted(targets) == list(range(R, H))


def test_option_is_validated(fr):
    K = fr._capi
    with pytest.raises(K.FractalRendererError):
        _fold(fr, *BIG, tunings=(("fold", 3),))
    with pytest.raises(K.FractalRendererError):
        _fold(fr, *BIG, tunings=(("fold", -1),))


@pytest.mark.parametrize("W", [1, 7, 250, 257, 1000, 4095, 4096, 65535])
def test_division_is_exact(fr, W):
    K = fr._capi
    top = (1 << 31) - 1                                     # the largest index of a legal frame
    magic, shift, ok = K.fold_division(W, min(W * 4096, 1 << 31))
    assert ok, "the host's own check over the first 4096 rows"
    assert 0 < magic < (1 << 32) and 31 <= shift <= 62
    div = lambda i: (i * magic) >> shift
    assert div(0) == 0 and div(top) == top // W
    rows = top // W
    # every multiple of W, one below and one above it: the first 4096 rows, 4096 rows spread over the range, the last 4096
    sample = set(range(1, min(rows, 4096) + 1)) | set(range(1, rows + 1, max(1, rows // 4096))) | set(range(max(1, rows - 4096), rows + 1))
    for q in sample:
        for i in (q * W - 1, q * W, q * W + 1):
            if 0 <= i <= top:
                assert div(i) == i // W, (W, i)


def test_division_check_refuses_what_it_cannot_vouch_for(fr):
    K = fr._capi
    assert K.fold_division(4096, 1 << 31)[2] is True
    with pytest.raises(K.FractalRendererError):
        K.fold_division(0, 16)
    assert K.fold_division(4096, (1 << 31) + 1)[2] is False, "beyond 2^31 indices the bound no longer holds"


@pytest.mark.parametrize("W,H", [(257, 130), (257, 129), (64, 24), (130, 2)])
@pytest.mark.parametrize("precision", [1, 0])
def test_the_oracle_frames_are_symmetric(oracle, W, H, precision):
    """what the fold rests on, on the CPU oracle: rows r and H - r are equal bit for bit with center_y = 0 -- the default
    view, and a zoom along the real axis with center_y = -0.0 -- and are not with center_y = 0.1"""
    import numpy as np
    mirrored = lambda a: np.array_equal(a[1:(H + 1) // 2], a[H - 1:H // 2:-1])
    for view in (dict(center_x=-0.5, center_y=0.0, zoom=3.0), dict(center_x=-1.401155, center_y=-0.0, zoom=1e-3)):
        ref = oracle.render(oracle.OracleParams(max_iterations=200, precision=precision, **view), W, H)
        assert all(mirrored(a) for a in (ref.iter, ref.nu, ref.rgba)), view
    if H > 2:
        ref = oracle.render(oracle.OracleParams(max_iterations=200, precision=precision, center_x=-0.5, center_y=0.1, zoom=3.0), W, H)
        assert not mirrored(ref.iter)
