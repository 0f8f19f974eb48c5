"""The folded render (option "fold", fr_plan.h: plan_fold) on the GPU.

A Mandelbrot frame with center_y == 0 renders its rows [0, R) and stores every finished pixel of row r at row H - r as well:
the two orbits are conjugates bit for bit, and the plain colour stage reads the escape index and |z|^2 alone.  So every plane
of a render with "fold" = 2 must equal the render with "fold" = 1 bit for bit, and both are held against the oracle within
the bars of test_gpu_parity.py.  Renderer.last_fold() says what a render did: R where it was folded, 0 elsewhere.

Shapes: 257 x 130 and 257 x 129 (even and odd H, ragged columns, a trip of one sub-tile), 250 x 190, 64 x 24 (R = 16: rows
16-23 are mirror targets and nothing else), 64 x 16 (R = 16 = H: not folded).  Schedules: fp64 and fp32; one pass; staged with
b0 = 32; the survivor stream in one class and in two, on the all-interior view and on the default view; cycle closing on and
off.  Then each plane alone, the post chain, host planes, and the store footprint in guard-banded planes (tests/guarded.py):
no element of the frame keeps the fill pattern, no guard element loses it.
"""
import numpy as np
import pytest

from guarded import GuardedPlanes
from test_gpu_parity import check_against, gpu_render, to_state

pytestmark = pytest.mark.gpu

DEFAULT = dict(center_x=-0.5, center_y=0.0, zoom=3.0)
INTERIOR = dict(center_x=-0.2, center_y=0.0, zoom=0.5)     # every sample runs to max_iter
OPTS = ("fold", "staging", "stage_first", "whole_blocks", "periodicity")
ONE_PASS = dict(staging=1)
STAGED = dict(staging=3, stage_first=32)
SHAPES = [(257, 130), (257, 129), (250, 190), (64, 24)]
MAX_ITER = 200


def rows_rendered(H):
    return (H // 2 + 1 + 7) // 8 * 8


def render(fr, renderer, p, W, H, fold, host=False, **opts):
    """planes and last_fold() of one render with cycle closing off (unless opts say otherwise)"""
    try:
        for k, v in dict(dict(fold=fold, periodicity=-1), **opts).items():
            renderer.set_option(k, v)
        planes = gpu_render(fr, renderer, p, W, H, host=host)
        return planes, renderer.last_fold()
    finally:
        for k in OPTS:
            renderer.set_option(k, 0)


_REFS = {}


def reference(oracle, p, W, H):
    """the oracle's planes, computed once per request and left alone"""
    key = (W, H, p.precision, p.max_iterations, p.center_x, p.center_y, p.zoom, p.post_chain)
    if key not in _REFS:
        ref = oracle.render(p, W, H)
        for a in (ref.iter, ref.nu, ref.rgba):
            a.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def folded_equals_unfolded(fr, renderer, oracle, p, W, H, want_fold=None, host=False, **opts):
    on, R = render(fr, renderer, p, W, H, 2, host, **opts)
    off, none = render(fr, renderer, p, W, H, 1, host, **opts)
    assert none == 0, "fold = 1 renders every row itself"
    assert R == (rows_rendered(H) if want_fold is None else want_fold)
    for a, b, what in zip(on, off, ("rgba", "nu", "iter")):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what + " differs from the render with fold = 1"
    ref = reference(oracle, p, W, H)
    check_against(p, ref.iter, ref.nu, ref.rgba, *on)
    return on


@pytest.mark.parametrize("schedule", [ONE_PASS, STAGED], ids=["one_pass", "staged"])
@pytest.mark.parametrize("precision", [1, 0], ids=["fp64", "fp32"])
@pytest.mark.parametrize("W,H", SHAPES)
def test_every_shape_precision_and_schedule(fr, renderer, oracle, W, H, precision, schedule):
    p = oracle.OracleParams(max_iterations=MAX_ITER, precision=precision, **DEFAULT)
    folded_equals_unfolded(fr, renderer, oracle, p, W, H, **schedule)
    assert renderer.last_stages() == (1 if schedule is ONE_PASS else 2)


@pytest.mark.parametrize("view", [INTERIOR, DEFAULT], ids=["interior", "default"])
@pytest.mark.parametrize("whole", [1, 2])
@pytest.mark.parametrize("precision", [1, 0], ids=["fp64", "fp32"])
def test_survivor_stream_in_one_class_and_in_two(fr, renderer, oracle, precision, whole, view):
    """the store of an interior whole block (store_interior) and the ring's records, retired and deferred"""
    p = oracle.OracleParams(max_iterations=MAX_ITER, precision=precision, **view)
    for W, H in ((257, 130), (257, 129)):
        on, R = render(fr, renderer, p, W, H, 2, whole_blocks=whole, **STAGED)
        blocks = renderer.last_whole_blocks()
        assert R == 72
        assert (blocks[0] > 0) == (whole == 2), blocks
        assert blocks[0] <= (256 // 8) * (72 // 8), "whole blocks come from the rows that are rendered and from no others"
        folded_equals_unfolded(fr, renderer, oracle, p, W, H, whole_blocks=whole, **STAGED)


@pytest.mark.parametrize("schedule", [ONE_PASS, STAGED], ids=["one_pass", "staged"])
@pytest.mark.parametrize("periodicity", [1, -1])
@pytest.mark.parametrize("precision", [1, 0], ids=["fp64", "fp32"])
def test_cycle_closing_on_and_off(fr, renderer, oracle, precision, periodicity, schedule):
    """periodicity = 1: the PERIOD instantiations of the tile kernel (one pass) and of the lane pool (staged)"""
    p = oracle.OracleParams(max_iterations=400, precision=precision, **DEFAULT)
    folded_equals_unfolded(fr, renderer, oracle, p, 257, 130, periodicity=periodicity, **schedule)
    if schedule is STAGED:
        assert renderer.last_pool_closing() == (1 if periodicity == 1 else 0)


@pytest.mark.parametrize("plane", ["rgba", "nu", "iter"])
@pytest.mark.parametrize("schedule", [ONE_PASS, STAGED], ids=["one_pass", "staged"])
def test_each_plane_alone(fr, renderer, oracle, schedule, plane):
    import torch
    W, H = 250, 190
    p = oracle.OracleParams(max_iterations=MAX_ITER, **DEFAULT)
    full, _ = render(fr, renderer, p, W, H, 1, **schedule)
    dev = torch.device("cuda:0")
    out = {"rgba": torch.full((H, W, 4), -7.0, dtype=torch.float32, device=dev),
           "nu": torch.full((H, W), -7.0, dtype=torch.float64, device=dev),
           "iter": torch.full((H, W), -7, dtype=torch.int32, device=dev)}[plane]
    torch.cuda.synchronize()
    try:
        for k, v in dict(dict(fold=2, periodicity=-1), **schedule).items():
            renderer.set_option(k, v)
        renderer.render(to_state(fr, p), W, H, **{plane: out})
        assert renderer.last_fold() == 96
    finally:
        for k in OPTS:
            renderer.set_option(k, 0)
    assert np.array_equal(out.cpu().numpy(), full[("rgba", "nu", "iter").index(plane)])


@pytest.mark.parametrize("schedule", [ONE_PASS, STAGED], ids=["one_pass", "staged"])
def test_post_chain(fr, renderer, oracle, schedule):
    p = oracle.OracleParams(max_iterations=MAX_ITER, post_chain=1, **DEFAULT)
    folded_equals_unfolded(fr, renderer, oracle, p, 257, 129, **schedule)
    pi = oracle.OracleParams(max_iterations=MAX_ITER, post_chain=1, **INTERIOR)
    folded_equals_unfolded(fr, renderer, oracle, pi, 257, 129, whole_blocks=2, **schedule)


@pytest.mark.parametrize("schedule", [ONE_PASS, STAGED], ids=["one_pass", "staged"])
def test_host_planes(fr, renderer, oracle, schedule):
    p = oracle.OracleParams(max_iterations=MAX_ITER, **DEFAULT)
    folded_equals_unfolded(fr, renderer, oracle, p, 257, 130, host=True, **schedule)


@pytest.mark.parametrize("schedule", [ONE_PASS, STAGED, dict(STAGED, whole_blocks=2)], ids=["one_pass", "staged", "staged_whole"])
@pytest.mark.parametrize("precision", [1, 0], ids=["fp64", "fp32"])
@pytest.mark.parametrize("W,H", [(257, 129), (257, 130), (64, 24), (7, 33)])
def test_store_footprint(fr, renderer, oracle, W, H, precision, schedule):
    """guard-banded planes filled with a pattern no kernel produces: the folded render leaves none of it inside the frame
    and all of it in the bands, and what it stored is the oracle's frame"""
    view = INTERIOR if "whole_blocks" in schedule else DEFAULT
    p = oracle.OracleParams(max_iterations=MAX_ITER, precision=precision, **view)
    g = GuardedPlanes(H, W, f64=precision == 1, backend="device")
    prec = fr.Precision.F64 if precision == 1 else fr.Precision.F32
    try:
        for k, v in dict(dict(fold=2, periodicity=-1), **schedule).items():
            renderer.set_option(k, v)
        renderer.render(to_state(fr, p), W, H, fractal_type=fr.FractalType(0), precision=prec, **g.kwargs())
        assert renderer.last_fold() == rows_rendered(H)
    finally:
        for k in OPTS:
            renderer.set_option(k, 0)
    assert g.guards_intact(), g.guard_hits()
    assert g.unwritten() == 0, "a pixel of the frame was never stored"
    ref = reference(oracle, p, W, H)
    check_against(p, ref.iter, ref.nu, ref.rgba, *g.values())


def test_frame_with_no_row_to_mirror_is_not_folded(fr, renderer, oracle):
    """64 x 16: R = 16 = H"""
    p = oracle.OracleParams(max_iterations=MAX_ITER, **DEFAULT)
    folded_equals_unfolded(fr, renderer, oracle, p, 64, 16, want_fold=0, **ONE_PASS)
    folded_equals_unfolded(fr, renderer, oracle, p, 64, 16, want_fold=0, **STAGED)


@pytest.mark.parametrize("schedule", [ONE_PASS, STAGED], ids=["one_pass", "staged"])
def test_view_off_the_real_axis_is_not_folded(fr, renderer, oracle, schedule):
    p = oracle.OracleParams(max_iterations=MAX_ITER, center_x=-0.5, center_y=0.1, zoom=3.0)
    folded_equals_unfolded(fr, renderer, oracle, p, 257, 130, want_fold=0, **schedule)
    tiny = oracle.OracleParams(max_iterations=MAX_ITER, center_x=-0.5, center_y=1e-300, zoom=3.0)
    folded_equals_unfolded(fr, renderer, oracle, tiny, 257, 130, want_fold=0, **schedule)
    negative_zero = oracle.OracleParams(max_iterations=MAX_ITER, center_x=-0.5, center_y=-0.0, zoom=3.0)
    folded_equals_unfolded(fr, renderer, oracle, negative_zero, 257, 130, want_fold=72, **schedule)


def test_other_requests_are_not_folded(fr, renderer, oracle):
    """Julia, Burning Ship, stripes, SSAA and a row-strip shard with fold = 2: last_fold() reads 0"""
    for kw in (dict(fractal=1, julia_c_real=-0.123, julia_c_imag=0.745), dict(fractal=2), dict(stripe_enabled=1), dict(aa=2)):
        p = oracle.OracleParams(max_iterations=64, center_x=0.0, center_y=0.0, zoom=3.0, **kw)
        _, R = render(fr, renderer, p, 64, 48, 2)
        assert R == 0, kw
    p = oracle.OracleParams(max_iterations=64, **DEFAULT)
    try:
        renderer.set_option("fold", 2)
        gpu_render(fr, renderer, p, 64, 48, shard=fr.Shard(0, 2, 8))
        assert renderer.last_fold() == 0
        gpu_render(fr, renderer, p, 64, 48)
        assert renderer.last_fold() == 32
    finally:
        renderer.set_option("fold", 0)


def test_automatic_setting_folds_from_two_to_the_twenty_pixels(fr, renderer, oracle):
    """520 x 504, the largest center_y = 0 frame whose schedule other tests pin, stays unfolded; 1024 x 1024 folds"""
    p = oracle.OracleParams(max_iterations=64, **DEFAULT)
    _, R = render(fr, renderer, p, 520, 504, 0)
    assert R == 0
    _, R = render(fr, renderer, p, 1024, 1023, 0)
    assert R == 0
    auto, R = render(fr, renderer, p, 1024, 1024, 0)
    assert R == 520
    off, none = render(fr, renderer, p, 1024, 1024, 1)
    assert none == 0
    for a, b in zip(auto, off):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    ref = reference(oracle, p, 1024, 1024)
    check_against(p, ref.iter, ref.nu, ref.rgba, *auto)


def test_folded_and_unfolded_renders_back_to_back(fr, renderer, oracle):
    """folded, off the axis, folded, without a host sync in between, three times: nothing of one render's geometry leaks
    into the next (the rows a folded render does not render are its predecessor's until the mirror stores land)"""
    import torch
    W, H = 257, 130
    views = [DEFAULT, dict(center_x=-0.5, center_y=0.1, zoom=3.0), INTERIOR]
    want = [render(fr, renderer, oracle.OracleParams(max_iterations=MAX_ITER, **v), W, H, 1, **STAGED)[0] for v in views]
    dev = torch.device("cuda:0")
    outs = [(torch.empty((H, W, 4), dtype=torch.float32, device=dev), torch.empty((H, W), dtype=torch.float64, device=dev),
             torch.empty((H, W), dtype=torch.int32, device=dev)) for _ in range(3)]
    torch.cuda.synchronize()
    folds = []
    try:
        for k, v in dict(dict(fold=2, periodicity=-1, whole_blocks=2), **STAGED).items():
            renderer.set_option(k, v)
        for rnd in range(3):
            for v, o in zip(views, outs):
                renderer.render(fr.FractalState(max_iterations=MAX_ITER, **v), W, H, rgba=o[0], nu=o[1], iter=o[2], sync=False)
                folds.append(renderer.last_fold())
        torch.cuda.synchronize()
        renderer.check()
    finally:
        for k in OPTS:
            renderer.set_option(k, 0)
    assert folds == [72, 0, 72] * 3
    for w, o in zip(want, outs):
        for a, b in zip(w, o):
            assert np.array_equal(a, b.cpu().numpy())
