"""What fr_plan_describe says is what enqueue_render does: the grid, the number of passes and whether the lane pool looks for
cycles of a dozen small renders -- one pass, staged, lean stripes, staged SSAA, a 2-part shard -- against the plan made
for the context's compute-unit count."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (W, H, fractal, f64, max_iter, aa, stripe, shard)
RENDERS = [
    (64, 64, "Mandelbrot", 0, 64, 1, 0, None),            # one pass
    (64, 64, "Mandelbrot", 1, 2048, 1, 0, None),          # staged
    (64, 64, "Mandelbrot", 0, 2048, 1, 1, None),          # lean stripes
    (64, 64, "JuliaSet", 0, 2048, 2, 0, None),               # staged SSAA
    (257, 129, "Mandelbrot", 0, 300, 1, 0, None),
    (257, 129, "JuliaSet", 1, 2048, 1, 0, None),
    (257, 129, "Mandelbrot", 1, 2048, 2, 0, None),
    (257, 129, "Mandelbrot", 0, 2048, 1, 0, (1, 2, 8)),   # a 2-part shard
    (520, 504, "BurningShip", 0, 200, 1, 0, None),
    (520, 504, "Mandelbrot", 0, 2048, 1, 0, None),
    (520, 504, "Mandelbrot", 1, 2048, 1, 1, None),
    (520, 504, "Mandelbrot", 0, 2048, 2, 0, None),
    (520, 504, "JuliaSet", 0, 2048, 1, 0, (0, 2, 12)),       # strips that are no whole sub-tile rows: the general kernel
]


@pytest.mark.parametrize("periodicity", [1, -1])
def test_plan_equals_execution(fr, periodicity):
    from fractalrenderer_amd import _capi
    seen = set()
    with fr.Renderer(0) as r:
        r.set_option("periodicity", periodicity)
        cu = r.compute_units
        for W, H, fractal, f64, max_iter, aa, stripe, sh in RENDERS:
            state = fr.FractalState(max_iterations=max_iter, antialiasing_samples=aa, stripe_enabled=bool(stripe))
            ftype, prec = getattr(fr.FractalType, fractal), (fr.Precision.F64 if f64 else fr.Precision.F32)
            shard = fr.Shard(*sh) if sh else None
            rows = shard.rows(H) if shard else H
            it = np.empty((rows, W), dtype=np.int32)
            r.render(state, W, H, fractal_type=ftype, precision=prec, iter=it, shard=shard)
            plan = _capi.plan_describe(state.to_params(ftype, prec), W, H, shard.to_c() if shard else None, cu,
                                       [("periodicity", periodicity)])
            what = (W, H, fractal, f64, max_iter, aa, stripe, sh)
            closing = -1 if plan["nstages"] < 2 else int(bool(plan["pool_may_look"]) and periodicity > 0)
            stages = plan["nstages_all"] if closing == 0 else plan["nstages"]
            assert (r.last_grid(), r.last_stages()) == (plan["grid"], stages), what
            assert r.last_pool_closing() == closing, what
            seen.add((plan["route"], plan["family"], plan["nstages"]))
    assert {(1, 3, 1), (1, 3, 2), (1, 4, 2), (3, 3, 2), (1, 0, 2)} <= seen, seen     # every kind of render above was one


def test_automatic_periodicity_asks_the_context_only_where_the_pool_may_look(fr):
    """periodicity 0: the first staged render of a fresh context looks (pool_wants_cycle_closing: LOOK); a lean-stripes
    render is never asked (pool_may_look 0) and does not look; a one-pass render has no pool"""
    with fr.Renderer(0) as r:
        it = np.empty((64, 64), dtype=np.int32)
        r.render(fr.FractalState(max_iterations=2048), 64, 64, precision=fr.Precision.F64, iter=it)
        assert (r.last_stages(), r.last_pool_closing()) == (2, 1)
        r.render(fr.FractalState(max_iterations=2048, stripe_enabled=True), 64, 64, precision=fr.Precision.F32, iter=it)
        assert (r.last_stages(), r.last_pool_closing()) == (2, 0)
        r.render(fr.FractalState(max_iterations=64), 64, 64, precision=fr.Precision.F32, iter=it)
        assert (r.last_stages(), r.last_pool_closing()) == (1, -1)
