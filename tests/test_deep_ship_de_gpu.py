"""fr_render_deep_ship_de on the GPU (fp64 deltas, zoom 1e-290 .. 1e3): the planes against tests/deep_ship_de_ref.py and against
fr_render_deep_ship, the edges, the shading, shards / layouts / memory kinds / the asynchronous form, and the state it shares with
fr_render_deep_ship.  The checks are tests/deep_ship_de_checks.py's, shared with the extended entry point's tests."""
import numpy as np
import pytest

import deep_ship_de_checks as K

pytestmark = pytest.mark.gpu
EXT = False
BLA = pytest.mark.parametrize("bla", [False, True], ids=["plain", "bla"])


@BLA
@pytest.mark.parametrize("name,w,h,aa", [("A", 48, 36, 1), ("B", 48, 36, 1), ("A", 32, 24, 3)], ids=["A", "B", "A-aa3"])
def test_planes_match_the_restatement_and_the_plain_entry_point(fr, renderer, name, w, h, aa, bla):
    v, samples, counts, got = K.check_case(fr, renderer, name, w, h, aa, bla, EXT)
    esc = samples[0][0] < v["max_iter"]
    assert esc.any() and not esc.all()
    j = got["deriv"][esc]
    assert (np.abs(j[:, 0] - j[:, 3]) > 1e-3 * np.abs(j).max(axis=1)).any()          # visibly not conformal
    if bla:
        assert counts[1] > 0


@BLA
@pytest.mark.parametrize("name", ["n1", "n2", "n3"])
def test_max_iterations_1_to_3(fr, renderer, name, bla):
    v, samples, counts, got = K.check_case(fr, renderer, name, 32, 24, 1, bla, EXT)
    it = samples[0][0]
    if name == "n1":                                               # an all-interior frame: every plane of the estimate is zero
        assert np.all(it == 1) and not got["de"].any() and not got["deriv"].any()
    else:
        assert (it < v["max_iter"]).any() and (it == v["max_iter"]).any()


@pytest.mark.parametrize("edge", [0.5, 1.8])
@pytest.mark.parametrize("aa,post,bla", [(1, False, False), (3, True, True)], ids=["aa1", "aa3-post-bla"])
def test_shading(fr, renderer, oracle, aa, post, bla, edge):
    K.check_shading(fr, renderer, oracle, "A", 32, 24, aa, edge, post, bla, EXT)


@BLA
def test_shards_layouts_memory_kinds_async_and_single_planes(fr, renderer, bla):
    K.check_plumbing(fr, renderer, "A", bla, EXT)


def test_orbit_table_and_step_counts_are_shared_with_fr_render_deep_ship(fr):
    K.check_shared_state(fr, "A", EXT)
