"""The Deep_Zoom cases (tests/deepzoom_cases.py) on the CPU: what each case can see, asserted on the oracle's output alone.
test_deepzoom_gpu.py holds the same cases to the oracle on the GPU; that a loop of deep_zoom_kernel which is off by one
update, one index or one group changes a pixel of them is decided here.  No GPU: the CPU oracle, and the product library's
host side for the reference length."""
import numpy as np
import pytest

import deepzoom_cases as dc


def _ids(cases):
    return dict(argvalues=list(cases), ids=list(cases))


def _census(case):
    """escapes per update, and the interior count, of the case's reference"""
    p = case[0]
    it = dc.reference(case).iter
    return [dc.escapes_at(it, i) for i in range(p.max_iterations)], dc.interior(it, p)


@pytest.mark.parametrize("cid", **_ids(dc.REMAINDER))
def test_remainder_cases_put_escapes_into_both_tails(cid):
    case = dc.REMAINDER[cid]
    p = case[0]
    m, r = int(cid[1]), int(cid[-1])
    L = dc.REMAINDER_VIEWS[m][1]
    assert dc.orbit_length(p) == L and L % 4 == m and p.max_iterations == L + r
    assert dc.ref_iter(p) == dc.n_ref(p) == L                      # the centre escapes: the orbit ends before max_iter
    assert list(dc.perturbed_tail(p)) == list(range(4 * (L // 4), L)) and list(dc.plain_phase(p)) == list(range(L, L + r))
    esc, inside = _census(case)
    print(cid, esc, inside)
    for i in dc.perturbed_tail(p):
        assert esc[i] >= 1, (cid, "perturbed tail", i)
    for i in dc.plain_phase(p):
        assert esc[i] >= 1, (cid, "plain phase", i)
    assert esc[p.max_iterations - 1] >= 1                         # the last update of all decides a pixel
    assert inside >= 1                                             # ... and some run through both phases to the end


def test_remainder_cases_cover_every_pair_of_remainders():
    pairs = {(dc.n_ref(p) % 4, len(dc.plain_phase(p)) % 4, len(dc.plain_phase(p)) >= 4) for p, _, _ in dc.REMAINDER.values()}
    assert pairs == {(a, b, full) for a in range(4) for b in range(4) for full in (False, True)}
    assert len(dc.REMAINDER) == 32
    # the third update of a full group of the perturbed phase decides pixels too (index 2 of a group)
    for m in (0,):
        esc, _ = _census(dc.REMAINDER[f"L{m}-r0"])
        assert esc[2] >= 1 and esc[6] >= 1 and esc[10] >= 1


@pytest.mark.parametrize("cid", **_ids(dc.INTERIOR_CENTRE))
def test_interior_centre_cases_have_no_plain_phase(cid):
    case = dc.INTERIOR_CENTRE[cid]
    p = case[0]
    assert dc.ref_iter(p) == dc.n_ref(p) == p.max_iterations and len(dc.plain_phase(p)) == 0
    esc, inside = _census(case)
    print(cid, esc, inside)
    assert all(n >= 1 for n in esc[1:]), (cid, esc)
    assert inside >= 100
    assert {c[0].max_iterations % 4 for c in dc.INTERIOR_CENTRE.values()} == {0, 1, 2, 3}


@pytest.mark.parametrize("cid", **_ids(dc.NO_ORBIT))
def test_no_orbit_cases_put_escapes_at_every_update(cid):
    case = dc.NO_ORBIT[cid]
    p = case[0]
    assert not p.use_perturbation and dc.ref_iter(p) == dc.n_ref(p) == 0
    assert list(dc.plain_phase(p)) == list(range(p.max_iterations))
    esc, inside = _census(case)
    print(cid, esc, inside)
    assert all(n >= 2 for n in esc), (cid, esc)
    assert inside >= 449
    assert {c[0].max_iterations for c in dc.NO_ORBIT.values()} == set(range(1, 10)) | {15, 16, 17}


@pytest.mark.parametrize("cid", **_ids(dc.RAGGED))
def test_ragged_cases_leave_lanes_without_a_sample(cid):
    p, W, H = case = dc.RAGGED[cid]
    assert W % dc.TILE or H % dc.TILE
    classes = np.unique(dc.reference(case).iter)
    print(cid, classes)
    if (W, H) != (1, 1):
        assert len(classes[classes < p.max_iterations]) >= 2, (cid, classes)
    else:
        assert dc.near_wrap(p, dc.reference(case).nu) == 0         # one pixel: its colour is held to the bar, no exception
    assert {(c[1], c[2]) for c in dc.RAGGED.values()} == set(dc.RAGGED_SIZES) and len(dc.RAGGED) == 10
    assert {(c[0].use_perturbation, c[0].max_iterations) for c in dc.RAGGED.values()} == {(1, 12), (0, 17)}


def test_wave_exit_cases_hold_dead_mixed_and_interior_blocks():
    census = {cid: dc.block_census(case) for cid, case in dc.WAVE_EXIT.items()}
    print(census)
    dead, mixed, inside = (sum(c[k] for c in census.values()) for k in range(3))
    assert dead >= 1 and mixed >= 1 and inside >= 1
    # as the issue found them: the escaping view brings the dead and the mixed blocks, the interior view the interior ones
    assert census["escaping-37"][0] >= 50 and census["escaping-37"][1] >= 6 and census["interior-9"][2] >= 16
    p = dc.WAVE_EXIT["escaping-37"][0]
    assert dc.n_ref(p) == 34 and len(dc.plain_phase(p)) == 3
    assert all((W, H) == (64, 64) for _, W, H in dc.WAVE_EXIT.values())


@pytest.mark.parametrize("view", list(dc.COLOUR_VIEWS))
@pytest.mark.parametrize("palette", dc.PALETTES)
def test_colour_cases_stay_clear_of_the_palette_wrap(view, palette):
    seen = 0
    for cid, key in dc.COLOUR_KEYS.items():
        if key[:2] != (view, palette):
            continue
        case = dc.COLOUR[cid]
        p, W, H = case
        ref = dc.reference(case)
        assert np.isfinite(ref.rgba).all() and np.isfinite(ref.nu).all() and np.all(ref.rgba[..., 3] == 1.0), cid
        if p.bailout == 3e19:                                      # bailout^2 is inf in float: nothing ever escapes
            with np.errstate(over="ignore"):
                assert np.isinf(np.float32(p.bailout) * np.float32(p.bailout))
            assert dc.interior(ref.iter, p) == W * H, cid
        else:
            assert 0 < dc.interior(ref.iter, p) < W * H // 4, cid
        if p.bailout == 0.5:                                       # clamped to 2
            two = dc.COLOUR[dc.colour_id(view, palette, key[2], key[3], 2.0)]
            assert np.array_equal(ref.iter, dc.reference(two).iter), cid
        near = dc.near_wrap(p, ref.nu)
        assert near <= dc.wrap_cap(W * H), (cid, near)
        seen += 1
    assert seen == len(dc.SCALE_OFFSET) * len(dc.BAILOUTS)


def test_colour_cases_are_the_issue_s_grid():
    assert len(dc.COLOUR) == 240 and dc.PALETTES == (-1, 0, 1, 2, 3, 4) and dc.BAILOUTS == (0.5, 2.0, 4.0, 1e4, 3e19)
    for view, (_, pairs) in dc.COLOUR_VIEWS.items():
        assert [sc for sc, _ in pairs] == [1.0, -2.5, 6.0, 0.0]             # one negative and one zero scale stay
    # a bailout below the clamp is visible: without the clamp (bailout 0.5 taken as written) samples would leave earlier
    for view, (make, _) in dc.COLOUR_VIEWS.items():
        it2 = dc.reference((make(bailout=2.0), dc.W0, dc.H0)).iter
        it4 = dc.reference((make(bailout=4.0), dc.W0, dc.H0)).iter
        assert (it2 != it4).mean() >= 0.05, view                            # ... as they leave earlier at 2 than at 4
    # every palette differs from every other on these frames, the fall-back (-1, 3, 4: one palette) aside
    for view, (make, pairs) in dc.COLOUR_VIEWS.items():
        sc, off = pairs[0]
        rgb = {m: dc.reference((make(palette_mode=m, color_scale=sc, color_offset=off), dc.W0, dc.H0)).rgba for m in dc.PALETTES}
        for a in (0, 1, 2, 3):
            for b in (0, 1, 2, 3):
                if a < b:
                    assert (np.abs(rgb[a] - rgb[b]).max(axis=2) > 1e-3).mean() >= 0.5, (view, a, b)
        assert np.array_equal(rgb[-1], rgb[3]) and np.array_equal(rgb[4], rgb[3])


def test_sweep_reaches_every_remainder_and_mixed_frames(fr):
    assert len(dc.SWEEP) == 32
    assert all(fr.Shard(*shard).rows(H) > 0 for _, _, H, shard in dc.SWEEP.values() if shard)
    nref, plain, mixed = set(), set(), 0
    for cid, (p, W, H, shard) in dc.SWEEP.items():
        assert p.fractal == 5 and p.max_iterations in dc.SWEEP_ITERS and p.bailout in dc.SWEEP_BAILOUTS
        assert -1 <= p.palette_mode <= 4 and 9 <= W <= 131 and 5 <= H <= 67
        assert (shard is not None) == (int(cid[-2:]) % 3 == 1)
        ref = dc.reference((p, W, H))
        nref.add(dc.n_ref(p) % 4)
        plain.add(len(dc.plain_phase(p)) % 4)
        mixed += 0 < dc.interior(ref.iter, p) < W * H
        assert dc.near_wrap(p, ref.nu) <= dc.wrap_cap(W * H), cid
    print(nref, plain, mixed)
    assert nref == {0, 1, 2, 3} and plain == {0, 1, 2, 3} and mixed >= 8
    assert {p.use_perturbation for p, _, _, _ in dc.SWEEP.values()} == {0, 1}
    assert any(W % 8 and H % 8 for _, W, H, _ in dc.SWEEP.values())


def test_orbit_sequence_puts_short_orbits_behind_long_ones():
    lengths = [dc.ref_iter(p) for p, _, _ in dc.ORBIT_SEQUENCE]
    print(lengths)
    assert lengths == [2000, 5, 0, 7, 3087, 5]                     # (the seahorse centre leaves after 3087 updates)
    assert dc.ORBIT_SEQUENCE[4][0].max_iterations > dc.ORBIT_SEQUENCE[0][0].max_iterations     # sized by max_iter: they grow
    # the short renders read past their own orbit if the kernel's bounds are wrong: what lies there is the seahorse orbit
    for p, _, _ in dc.ORBIT_SEQUENCE[1:4]:
        assert p.max_iterations > dc.ref_iter(p)


def _perturbed_cases():
    for group, cases in dc.GROUPS.items():
        for cid, (p, _, _) in cases.items():
            if p.use_perturbation:
                yield group + "/" + cid, p
    for k, (p, _, _) in enumerate(dc.ORBIT_SEQUENCE):
        if p.use_perturbation:
            yield "sequence/%d" % k, p


def test_reference_length_in_the_push_constants(fr, oracle):
    """reference_iterations (slot 13 of the Deep_Zoom push constants) as the product's host side computes it, for every
    perturbed case: the length of the oracle's reference orbit, which is where the kernel's two phases join."""
    from test_gpu_parity import to_state
    n = 0
    for cid, p in _perturbed_cases():
        want = len(oracle.reference_orbit(p.center_x, p.center_y, p.max_iterations))
        got = fr.pack_push_constants(to_state(fr, p), fr.FractalType.Deep_Zoom)
        assert got[13] == np.float32(want) and want == dc.ref_iter(p), (cid, float(got[13]), want)
        assert got[6] == np.float32(p.max_iterations) and got[7] == 1.0
        n += 1
    assert n >= 32 + 9 + 5 + 2 + 120


def test_no_frame_needs_more_colour_than_the_bar_gives():
    """RGB_TOL is a bar on the colour stage's own arithmetic; one ulp of the palette's fract argument must fit under it, or a
    frame fails on the float rounding of t * k wherever nu itself differs by an ulp (see deepzoom_cases.seahorse)."""
    from test_gpu_parity import RGB_TOL
    frames = [(g + "/" + cid, p) for g, cases in dc.GROUPS.items() for cid, (p, _, _) in cases.items()]
    frames += [("sequence/%d" % k, p) for k, (p, _, _) in enumerate(dc.ORBIT_SEQUENCE)]
    worst = max(frames, key=lambda f: dc.colour_ulp(f[1]))
    print(worst[0], dc.colour_ulp(worst[1]))
    assert dc.colour_ulp(worst[1]) <= RGB_TOL / 2, worst[0]
    # ... which palette 0 at the seahorse frames' iteration counts would not
    p0 = dc.seahorse(2000)
    p0.palette_mode = 0
    assert dc.colour_ulp(p0) > RGB_TOL
