"""The render schedule, pinned without a GPU.

None of the planner's thresholds (fr_plan.h: staging_threshold, plan_stages, plan_tile_queue, the lean predicates, the SSAA
routes) can change a pixel, so the GPU suite passes whichever schedule is chosen.  tests/golden/render_plans.npz records what
the library decided for every request of render_plan_cases.py before the planner was pulled out of enqueue_render (commit
e435e45, its enqueue_render(reserve_only) made to write its decisions out on a context without a device);
fr_plan_describe must reproduce every row exactly.  A change of schedule is then a change of this fixture, made on purpose.

Re-recording after such a change: fr_plan_describe is then the only source.  Build the commit BEFORE the change, describe
every request of render_plan_cases.cases() with it (this file's _describe), do the same with the commit after it, and review
the rows that differ -- they must be the intended ones and no others -- before saving fields / requests / tunings / plans
with numpy.savez_compressed.  New requests go at the end of a block of cases(), so that old rows keep their meaning.
"""
import os

import numpy as np
import pytest

import render_plan_cases as RC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_plans.npz")


@pytest.fixture(scope="module")
def recorded():
    return np.load(GOLDEN)


def _describe(fr, case):
    from fractalrenderer_amd import _capi
    fractal, f64, max_iter, aa, trap, stripe, interior, W, H, part, nparts, rps, cu = (int(v) for v in case[:13])
    p = _capi.fr_params()
    _capi.check(_capi.lib().fr_params_default(p))
    p.fractal_type, p.precision, p.max_iterations, p.antialiasing_samples = fractal, f64, max_iter, aa
    p.orbit_trap_enabled, p.stripe_enabled, p.interior_style = trap, stripe, interior
    shard = _capi.fr_shard(part, nparts, rps) if nparts else None
    return _capi.plan_describe(p, W, H, shard, cu, RC.parse_tunings(str(case[13])))


def test_fixture_holds_the_case_matrix(recorded):
    cases = RC.cases()
    assert recorded["requests"].shape == (len(cases), 13) and recorded["plans"].shape[0] == len(cases)
    assert np.array_equal(recorded["requests"], np.array([c[:13] for c in cases], dtype=np.int64))
    assert [str(t) for t in recorded["tunings"]] == [c[13] for c in cases]
    folder = os.path.dirname(GOLDEN)         # no larger than the largest of the other fixtures
    assert os.path.getsize(GOLDEN) <= max(os.path.getsize(os.path.join(folder, f)) for f in os.listdir(folder) if f != "render_plans.npz")


def test_matrix_straddles_the_thresholds(recorded):
    """every value a threshold can produce is in the record: both sides of each were reached"""
    fields = [str(f) for f in recorded["fields"]]
    plans = recorded["plans"]
    col = lambda name: set(int(v) for v in plans[:, fields.index(name)])
    assert col("route") == {1, 2, 3, 4}
    assert col("family") == {0, 1, 2, 3, 4}
    assert col("nstages") == {0, 1, 2} and (2, 1) in set(zip(plans[:, fields.index("nstages")], plans[:, fields.index("nstages_all")])) and col("wg_per_cu") >= {5, 6}
    assert col("tq_ns_log2") >= {3, 6} and col("pq_ns_log2") >= {3, 6}
    assert col("tq_nsx_shift") >= {-1, 0, 3, 6} and col("bounded") == {0, 1} and col("moderate") == {0, 1}
    assert col("b0_look") >= {16, 32, 48, 64, 96, 192} and col("b0_all") >= {96, 112, 176, 192}
    assert 0 in col("tq_flags") and 0 in col("pq_flags") and len(col("tq_flags")) >= 3
    assert col("tile_pixels") == {0, 1, 2} and col("shape") >= {3, 4, 6}
    requests = recorded["requests"]
    npx = set(int(w) * int(h) for w, h in requests[:, 7:9])
    for k in (18, 19, 20, 23, 24):
        assert {(1 << k) - 1, 1 << k, (1 << k) + 1} <= npx


def test_fr_plan_describe_reproduces_every_recorded_plan(fr, recorded):
    fields = [str(f) for f in recorded["fields"]]
    from fractalrenderer_amd import _capi
    assert _capi.lib().fr_plan_fields().decode().split() == fields
    wrong = []
    for i, (req, tun, want) in enumerate(zip(recorded["requests"], recorded["tunings"], recorded["plans"])):
        got = _describe(fr, list(req) + [tun])
        diff = {f: (int(w), got[f]) for f, w in zip(fields, want) if got[f] != int(w)}
        if diff:
            wrong.append((i, [int(v) for v in req], str(tun), diff))
    assert not wrong, f"{len(wrong)} of {len(recorded['plans'])} plans differ (field: (recorded, now)); the first: {wrong[:3]}"


def test_describe_rejects_what_the_setters_reject(fr):
    from fractalrenderer_amd import _capi
    p = _capi.fr_params()
    _capi.check(_capi.lib().fr_params_default(p))
    for tunings in ([("no_such_knob", 1)], [("regions", 16)], [("shards", 7)], [("debug_prologue_epoch", 5)]):
        with pytest.raises(_capi.FractalRendererError):
            _capi.plan_describe(p, 64, 64, None, 256, tunings)
    with pytest.raises(_capi.FractalRendererError):
        _capi.plan_describe(p, 64, 64, _capi.fr_shard(2, 2, 0), 256)
    assert _capi.plan_describe(p, 64, 8, _capi.fr_shard(1, 2, 8), 256)["route"] == 0      # a part that owns no rows
