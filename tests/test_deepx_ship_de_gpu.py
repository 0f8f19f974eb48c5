"""fr_render_deepx_ship_de on the GPU (extended deltas, zoom 1e-1000 .. 1e3): the planes against tests/deep_ship_de_ref.py and
against fr_render_deepx_ship on structured views, the tip of the needle (Y = 0 exactly, and Y tiny), an all-interior nucleus; the
bits of fr_render_deep_ship_de on views a double holds; the edges, the shading, the plumbing and the shared state.  The checks
are tests/deep_ship_de_checks.py's."""
import numpy as np
import pytest

import deep_ship_de_checks as K

pytestmark = pytest.mark.gpu
EXT = True
BLA = pytest.mark.parametrize("bla", [False, True], ids=["plain", "bla"])


@BLA
@pytest.mark.parametrize("name,w,h,aa", [("S310", 48, 36, 1), ("S400", 48, 36, 1), ("TIP400", 48, 36, 1), ("TIPY300", 48, 36, 1),
                                         ("S400", 32, 24, 3)], ids=["S310", "S400", "TIP400", "TIPY300", "S400-aa3"])
def test_planes_match_the_restatement_and_the_plain_entry_point(fr, renderer, name, w, h, aa, bla):
    v, samples, counts, got = K.check_case(fr, renderer, name, w, h, aa, bla, EXT)
    it = samples[0][0]
    esc = it < v["max_iter"]
    assert esc.any()
    assert np.all(np.isfinite(got["de"])) and np.all(got["de"][esc] > 0.0)           # finite at any depth
    if name.startswith("TIP"):
        # below the axis y is negative in one update: the pixels there carry J22 < 0 where those above carry J22 > 0
        j22 = got["deriv"][..., 3]
        assert (j22[esc] < 0.0).any() and (j22[esc] > 0.0).any()


@BLA
def test_an_all_interior_frame(fr, renderer, bla):
    v, samples, counts, got = K.check_case(fr, renderer, "NUC546", 48, 36, 1, bla, EXT)
    assert np.all(samples[0][0] == v["max_iter"]) and not got["de"].any() and not got["deriv"].any()


@BLA
@pytest.mark.parametrize("name", ["n1", "n2", "n3"])
def test_max_iterations_1_to_3(fr, renderer, name, bla):
    v, samples, counts, got = K.check_case(fr, renderer, name, 32, 24, 1, bla, EXT)
    it = samples[0][0]
    if name == "n1":
        assert np.all(it == 1) and not got["de"].any() and not got["deriv"].any()
    else:
        assert (it < v["max_iter"]).any() and (it == v["max_iter"]).any()


@BLA
@pytest.mark.parametrize("name", ["A", "B"])
def test_views_a_double_holds_get_the_bits_of_fr_render_deep_ship_de(fr, renderer, name, bla):
    w, h = 48, 36
    K.check_case(fr, renderer, name, w, h, 1, bla, EXT)
    got = K.render_de(fr, renderer, K.view_of(name, True), w, h, True, bla=bla)
    want = K.render_de(fr, renderer, K.view_of(name, False), w, h, False, bla=bla)
    for k in K.NAMES:
        assert K.same_bytes(got[k], want[k]), k
    assert want["deriv"].any() and (want["de"] > 0.0).any()


@pytest.mark.parametrize("edge", [0.5, 1.8])
@pytest.mark.parametrize("aa,post,bla", [(1, False, False), (3, True, True)], ids=["aa1", "aa3-post-bla"])
def test_shading(fr, renderer, oracle, aa, post, bla, edge):
    K.check_shading(fr, renderer, oracle, "S400", 32, 24, aa, edge, post, bla, EXT)


@BLA
def test_shards_layouts_memory_kinds_async_and_single_planes(fr, renderer, bla):
    K.check_plumbing(fr, renderer, "S400", bla, EXT)


def test_orbit_table_and_step_counts_are_shared_with_fr_render_deepx_ship(fr):
    K.check_shared_state(fr, "S310", EXT)
