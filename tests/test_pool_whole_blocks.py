"""The survivor stream in two classes (tuning "whole_blocks", fr_kernels.hip.h: WholeRef).

A full trip of the staged lean tile pass that lost no sample writes its records as whole blocks; the lane pool runs such a
block in a loop of its own -- exactly the updates it has left, unchecked -- and stores the interior result, or, when a stretch
comes out dirty, turns the 64 samples into running lanes and goes on as the lane pool always has.  Only where a sample's
updates run changes, so every plane must equal the render with "whole_blocks" = 1 bit for bit; one case per view is also held
against the general tile kernel and against the oracle, within the bars of test_gpu_parity.py.  The read-out
(Renderer.last_whole_blocks: whole blocks written, whole blocks that turned dirty, records through the ring) says which
paths a case took.  Sharded renders (row strips) and the sample grid of a staged SSAA frame take the path like any other
render: a record carries its pixel's place.
Every frame is 256 x 192 or smaller; staging is forced ("staging" = 3) and b0 set with "stage_first".
"""
import numpy as np
import pytest

from test_gpu_parity import check_against, gpu_render

MIXED = dict(center_x=-0.75, center_y=0.1, zoom=0.6)       # whole patches, some dirty later, and partial ones
INTERIOR = dict(center_x=-0.2, center_y=0.0, zoom=0.5)     # every patch whole, the ring's class empty
EXTERIOR = dict(center_x=8.0, center_y=8.0, zoom=2.0)      # no survivor in either class
OPTS = ("staging", "stage_first", "whole_blocks", "periodicity", "tile_kernel", "prepare", "stripes", "ssaa")


def render(fr, renderer, p, W, H, b0=32, whole=2, shard=None, **opts):
    """planes and read-out of one staged render with cycle closing off (unless opts say otherwise)"""
    try:
        for k, v in dict(dict(staging=3, stage_first=b0, whole_blocks=whole, periodicity=-1), **opts).items():
            renderer.set_option(k, v)
        planes = gpu_render(fr, renderer, p, W, H, shard=shard)
        return planes, renderer.last_whole_blocks()
    finally:
        for k in OPTS:
            renderer.set_option(k, 0)


def on_equals_off(fr, renderer, p, W, H, b0=32, shard=None, **opts):
    on, counts = render(fr, renderer, p, W, H, b0, 2, shard, **opts)
    off, none = render(fr, renderer, p, W, H, b0, 1, shard, **opts)
    assert none == (0, 0, 0), "whole_blocks = 1 keeps one class"
    for a, b, what in zip(on, off, ("rgba", "nu", "iter")):
        assert np.array_equal(a, b), what + " differs from the render with whole_blocks = 1"
    return on, counts


def against_general_kernel_and_oracle(fr, renderer, oracle, p, W, H, planes, b0=32):
    general, _ = render(fr, renderer, p, W, H, b0, 1, tile_kernel=1)
    for a, b in zip(planes, general):
        assert np.array_equal(a, b)
    ref = oracle.render(p, W, H)
    check_against(p, ref.iter, ref.nu, ref.rgba, *planes)
    return ref


@pytest.mark.gpu
def test_mixed_view_takes_all_three_paths(fr, renderer, oracle):
    p = oracle.OracleParams(max_iterations=400, **MIXED)
    planes, (whole, dirty, ring) = on_equals_off(fr, renderer, p, 256, 192)
    assert whole > 0 and dirty > 0 and ring > 0
    assert dirty < whole
    against_general_kernel_and_oracle(fr, renderer, oracle, p, 256, 192, planes)


@pytest.mark.gpu
def test_all_interior_view_leaves_the_ring_empty(fr, renderer, oracle):
    p = oracle.OracleParams(max_iterations=256, **INTERIOR)
    planes, (whole, dirty, ring) = on_equals_off(fr, renderer, p, 256, 192)
    assert whole == 256 * 192 // 64 and dirty == 0 and ring == 0
    ref = against_general_kernel_and_oracle(fr, renderer, oracle, p, 256, 192, planes)
    assert np.all(ref.iter == 256), "the interior view has escaping samples: it no longer tests what it is for"


@pytest.mark.gpu
def test_all_exterior_view_has_no_survivor(fr, renderer, oracle):
    p = oracle.OracleParams(max_iterations=400, **EXTERIOR)
    planes, counts = on_equals_off(fr, renderer, p, 256, 192)
    assert counts == (0, 0, 0)
    against_general_kernel_and_oracle(fr, renderer, oracle, p, 256, 192, planes)


@pytest.mark.gpu
def test_ragged_frame(fr, renderer, oracle):
    """250 x 190: edge columns and rows; the last trip of a row has one sub-tile and must take the ring"""
    p = oracle.OracleParams(max_iterations=300)
    planes, (whole, dirty, ring) = on_equals_off(fr, renderer, p, 250, 190, b0=48)
    assert whole > 0 and ring > 0 and dirty > 0
    against_general_kernel_and_oracle(fr, renderer, oracle, p, 250, 190, planes, b0=48)


@pytest.mark.gpu
@pytest.mark.parametrize("b0,max_iter", [(32, 383), (32, 400), (32, 401), (32, 415), (32, 64), (32, 79), (16, 32), (16, 33), (16, 47)])
def test_remaining_counts(fr, renderer, oracle, b0, max_iter):
    """Updates left to the pool that are no multiple of 16 or 64, and the fewest a staged frame can leave it: the planner
    stages a forced schedule from max_iter >= 2 b0 and b0 is a multiple of 16, so max_iter - b0 < 16 does not occur; the
    single-step remainder of the whole-block loop runs in 33, 47, 79 (1 and 15 mod 16) and in 383, 401, 415."""
    p = oracle.OracleParams(max_iterations=max_iter, **MIXED)
    _, (whole, dirty, ring) = on_equals_off(fr, renderer, p, 256, 192, b0=b0)
    assert whole > 0 and ring > 0
    if b0 == 32:
        assert dirty > 0          # the way back into the lane pool with these counts left, the single-step tail included


@pytest.mark.gpu
@pytest.mark.parametrize("interior_style", [0, 1, 2])
@pytest.mark.parametrize("post_chain", [0, 1])
def test_interior_colour_and_post_chain(fr, renderer, oracle, interior_style, post_chain):
    """interior_style 2 is an effects render (lean stripes instantiations): the plan keeps the path off"""
    p = oracle.OracleParams(max_iterations=400, interior_style=interior_style, post_chain=post_chain, **MIXED)
    planes, (whole, dirty, ring) = on_equals_off(fr, renderer, p, 256, 192)
    assert (whole > 0) == (interior_style != 2)
    if interior_style != 2:
        ref = oracle.render(p, 256, 192)
        check_against(p, ref.iter, ref.nu, ref.rgba, *planes)


@pytest.mark.gpu
@pytest.mark.parametrize("planes", ["rgba", "nu", "iter"])
def test_single_planes(fr, renderer, oracle, planes):
    import torch
    W, H = 256, 192
    st = fr.FractalState(max_iterations=400, **MIXED)
    full, _ = render(fr, renderer, oracle.OracleParams(max_iterations=400, **MIXED), W, H)
    dev = torch.device("cuda:0")
    out = {"rgba": torch.full((H, W, 4), -7.0, dtype=torch.float32, device=dev),
           "nu": torch.full((H, W), -7.0, dtype=torch.float64, device=dev),
           "iter": torch.full((H, W), -7, dtype=torch.int32, device=dev)}[planes]
    torch.cuda.synchronize()
    try:
        for k, v in dict(staging=3, stage_first=32, whole_blocks=2, periodicity=-1).items():
            renderer.set_option(k, v)
        renderer.render(st, W, H, **{planes: out})
        whole, _, _ = renderer.last_whole_blocks()
    finally:
        for k in OPTS:
            renderer.set_option(k, 0)
    assert whole > 0
    assert np.array_equal(out.cpu().numpy(), full[("rgba", "nu", "iter").index(planes)])


@pytest.mark.gpu
def test_fp32_and_julia_take_the_path(fr, renderer, oracle):
    """pool_kernel<float, 0, false> and <float / double, 1, false>: the plan sets the flag for every staged lean render
    whose pool neither looks for cycles nor shades stripes, whatever the precision and the fractal"""
    for kw in (dict(precision=0, max_iterations=400, **MIXED),
               dict(fractal=1, precision=0, center_x=0.0, center_y=0.0, zoom=3.0, max_iterations=272, julia_c_real=-0.123, julia_c_imag=0.745),
               dict(fractal=1, precision=1, center_x=0.0, center_y=0.0, zoom=3.0, max_iterations=272, julia_c_real=-0.123, julia_c_imag=0.745),
               dict(fractal=2, precision=1, center_x=-1.75, center_y=-0.03, zoom=0.1, max_iterations=272)):
        p = oracle.OracleParams(**kw)
        planes, (whole, dirty, ring) = on_equals_off(fr, renderer, p, 256, 192)
        if kw.get("fractal", 0) != 2:
            assert whole > 0, kw
            ref = oracle.render(p, 256, 192)
            check_against(p, ref.iter, ref.nu, ref.rgba, *planes)


@pytest.mark.gpu
@pytest.mark.parametrize("prepare", [0, 1])
def test_no_stale_counter(fr, renderer, oracle, prepare):
    """mixed, all exterior, all interior, back to back on one context without a host sync, three times: a counter of the second
    class that was not zeroed (in the tile pass's prologue; prepare = 1: by prepare_kernel) shows in the planes or the read-out"""
    import torch
    W, H = 256, 192
    views = [(MIXED, 400), (EXTERIOR, 400), (INTERIOR, 256)]
    want = [render(fr, renderer, oracle.OracleParams(max_iterations=mi, **v), W, H, whole=1)[0] for v, mi in views]
    dev = torch.device("cuda:0")
    outs = [[(torch.empty((H, W, 4), dtype=torch.float32, device=dev), torch.empty((H, W), dtype=torch.float64, device=dev),
              torch.empty((H, W), dtype=torch.int32, device=dev)) for _ in views] for _ in range(3)]
    torch.cuda.synchronize()
    try:
        for k, v in dict(staging=3, stage_first=32, whole_blocks=2, periodicity=-1, prepare=prepare).items():
            renderer.set_option(k, v)
        for rnd in range(3):
            for (v, mi), o in zip(views, outs[rnd]):
                renderer.render(fr.FractalState(max_iterations=mi, **v), W, H, rgba=o[0], nu=o[1], iter=o[2], sync=False)
        counts = renderer.last_whole_blocks()                # waits for the last render: the all-interior view
    finally:
        for k in OPTS:
            renderer.set_option(k, 0)
    assert counts == (W * H // 64, 0, 0)
    for rnd in range(3):
        for w, o in zip(want, outs[rnd]):
            for a, b in zip(w, o):
                assert np.array_equal(a, b.cpu().numpy())


@pytest.mark.gpu
def test_row_strips_take_the_path(fr, renderer, oracle):
    """2 parts, 8 rows per strip: a sharded render writes whole blocks like any other"""
    p = oracle.OracleParams(max_iterations=400, **MIXED)
    total = 0
    for part in range(2):
        _, (whole, dirty, ring) = on_equals_off(fr, renderer, p, 256, 192, shard=fr.Shard(part, 2, 8))
        total += whole
    assert total > 0


@pytest.mark.gpu
def test_periodicity_and_stripes_keep_the_path_off(fr, renderer, oracle):
    p = oracle.OracleParams(max_iterations=400, **MIXED)
    for periodicity in (0, 1):
        planes, counts = render(fr, renderer, p, 256, 192, periodicity=periodicity)
        if renderer.last_pool_closing() == 1 or periodicity == 1:
            assert counts == (0, 0, 0)
        off, _ = render(fr, renderer, p, 256, 192, whole=1)
        for a, b in zip(planes, off):
            assert np.array_equal(a, b)
    ps = oracle.OracleParams(max_iterations=400, stripe_enabled=1, **MIXED)
    _, counts = on_equals_off(fr, renderer, ps, 256, 192)
    assert counts == (0, 0, 0)


@pytest.mark.gpu
def test_staged_ssaa_sample_grid_takes_the_path(fr, renderer, oracle):
    """128 x 96 at 2 x 2 samples: the 256 x 192 sample grid goes through tile pass + lane pool like a frame of its own, whole
    blocks included; against the same render with one class, and against the sample loop of the general tile kernel"""
    p = oracle.OracleParams(max_iterations=400, aa=2, **MIXED)
    planes, (whole, dirty, ring) = on_equals_off(fr, renderer, p, 128, 96, ssaa=2)
    assert whole > 0 and ring > 0
    loop, none = render(fr, renderer, p, 128, 96, whole=2, ssaa=1)
    assert none == (0, 0, 0)
    for a, b in zip(planes, loop):
        assert np.array_equal(a, b)
