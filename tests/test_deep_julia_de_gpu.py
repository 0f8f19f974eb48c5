"""Distance estimates for deep Julia views on the GPU, fp64 deltas (fr_render_deep_julia_de): the five planes against the numpy
restatement (tests/deep_julia_de_ref.py) and against fr_render_deep_julia, plain and with FR_FLAG_DEEP_JULIA_BLA; against the
extended entry point; the edges; the shading; shards, layouts, memory kinds, the asynchronous form; and the caches it shares
with fr_render_deep_julia.  The checks are in tests/deep_julia_de_checks.py, shared with test_deepx_julia_de_gpu.py."""
import pytest

import deep_julia_de_checks as K

pytestmark = pytest.mark.gpu

EXT = False
CASES = [("RABBIT30", 48, 36, 1), ("DENDRITE30", 48, 36, 1), ("DUST30", 48, 36, 1), ("DENDRITE30", 48, 36, 2),
         ("DENDRITE100", 32, 24, 1), ("PRECRIT60", 32, 24, 1)]
EDGE_NAMES = ["n1", "n2", "n3", "np1", "np2", "np3", "esc0", "b0.75", "b65536"]
BLA = pytest.mark.parametrize("bla", [False, True], ids=["plain", "bla"])


@BLA
@pytest.mark.parametrize("name,w,h,aa", CASES, ids=["%s-%dx%d-aa%d" % c for c in CASES])
def test_planes_match_the_restatement_and_fr_render_deep_julia(fr, renderer, name, w, h, aa, bla):
    """RABBIT30 has an interior, the dendrites and the dust none; DUST30's filaments are far thinner than a pixel; PRECRIT60's
    samples step on both tables"""
    v, _, samples, counts, got = K.check_case(fr, renderer, name, w, h, aa, bla, EXT)
    if bla and name in ("RABBIT30", "DENDRITE100", "PRECRIT60"):
        assert counts[1] > 0


@pytest.mark.parametrize("name", ["RABBIT30", "DENDRITE100"])
def test_the_two_entry_points_write_the_same_de_and_deriv(fr, renderer, name):
    """the unflagged fp64 and extended renders of a view both accept: d0 is at least 2^-400 and no intermediate leaves a
    double's range, so de and deriv are byte-identical"""
    v, _ = K.view_of(name, False)
    w, h = 48, 36
    a = K.render_de(fr, renderer, v, w, h, False)
    b = K.render_de(fr, renderer, v, w, h, True)
    for k in ("iter", "de", "deriv"):
        assert K.same_bytes(a[k], b[k]), k
    assert (a["de"] > 0.0).any()


@BLA
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edges(fr, renderer, name, bla):
    K.check_edge(fr, renderer, name, bla, EXT)


@BLA
@pytest.mark.parametrize("aa", [1, 2])
@pytest.mark.parametrize("post", [False, True], ids=["linear", "post"])
@pytest.mark.parametrize("edge", [1.8, 0.25])
def test_shading(fr, renderer, oracle, edge, post, aa, bla):
    K.check_shading(fr, renderer, oracle, "DENDRITE30", 48, 36, aa, edge, post, bla, EXT)


@BLA
def test_shards_layouts_memory_and_async(fr, renderer, bla):
    K.check_plumbing(fr, renderer, "DENDRITE30", bla, EXT)


def test_caches_are_fr_render_deep_julias_own(fr):
    K.check_shared_state(fr, "DENDRITE100", EXT)
