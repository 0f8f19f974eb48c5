"""Distance estimates for deep Julia views on the GPU, extended deltas (fr_render_deepx_julia_de): the five planes against the
numpy restatement (tests/deep_julia_de_ref.py) and against fr_render_deepx_julia, plain and with FR_FLAG_DEEPX_JULIA_BLA; the
edges, the flush of the derivative among them; the shading; shards, layouts, memory kinds, the asynchronous form; and the caches
it shares with fr_render_deepx_julia.  The checks are in tests/deep_julia_de_checks.py, shared with test_deep_julia_de_gpu.py,
which also compares the two entry points with each other."""
import numpy as np
import pytest

import deep_julia_de_checks as K

pytestmark = pytest.mark.gpu

EXT = True
CASES = [("DENDRITE400", 48, 36, 1), ("DENDRITE1000", 32, 24, 1), ("PRECRIT200", 32, 24, 1), ("DUST30", 32, 24, 2)]
EDGE_NAMES = ["n1", "n2", "n3", "np1", "np2", "np3", "esc0", "b0.75", "b65536", "basin"]
BLA = pytest.mark.parametrize("bla", [False, True], ids=["plain", "bla"])


@BLA
@pytest.mark.parametrize("name,w,h,aa", CASES, ids=["%s-%dx%d-aa%d" % c for c in CASES])
def test_planes_match_the_restatement_and_fr_render_deepx_julia(fr, renderer, name, w, h, aa, bla):
    """the dendrites at 1e-400 and 1e-1000 start extended and turn plain; PRECRIT200's derivative drops by about 650 binades in
    one update and climbs back; DUST30 runs plain from the start, with aa 2"""
    v, _, samples, counts, got = K.check_case(fr, renderer, name, w, h, aa, bla, EXT)
    esc = samples[0][0] < v["max_iter"]
    if bla and name != "DUST30":
        assert counts[1] > 0 and counts[2] > counts[0]
    if name == "DENDRITE1000":                                    # de stays finite where deriv has left a double's range
        assert np.all(np.isfinite(got["de"][esc])) and np.all(got["de"][esc] > 0.0)
    if name == "PRECRIT200":
        assert esc.mean() >= 0.9


@BLA
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edges(fr, renderer, name, bla):
    K.check_edge(fr, renderer, name, bla, EXT)


@BLA
@pytest.mark.parametrize("aa", [1, 2])
@pytest.mark.parametrize("post", [False, True], ids=["linear", "post"])
@pytest.mark.parametrize("edge", [1.8, 0.25])
def test_shading(fr, renderer, oracle, edge, post, aa, bla):
    K.check_shading(fr, renderer, oracle, "DENDRITE400", 32, 24, aa, edge, post, bla, EXT)


@BLA
def test_shards_layouts_memory_and_async(fr, renderer, bla):
    K.check_plumbing(fr, renderer, "DENDRITE400", bla, EXT)


def test_caches_are_fr_render_deepx_julias_own(fr):
    K.check_shared_state(fr, "DENDRITE400", EXT)
