"""tests/field_build_reference.py - the exact reference the device-built likelihood field is held to - checked without a device:

  * it reproduces the reference project's own field pins (the ones tests/test_gpu_field_build.py quotes), at their tolerances;
  * its window minimum is the brute-force minimum over all seeds;
  * it equals the oracle's wavefront bit for bit where the wavefront is exact (one seed; single seeds farther apart than twice the cap);
  * it is never the smaller likelihood than the wavefront's on a rooms map and on turtlebot3;
  * the cases of the GPU suite can SEE what they check: every two different values a case's field can hold are at least 64 float32 steps
    apart (a condition on the parameters, fixed before any kernel ran) - and sigma_hit = 0.2 fails that condition;
  * the tie cases do hold cells whose admissible set has more than one member, and none at a dyadic resolution.
"""
import math
import os

import numpy as np
import pytest

import field_build_families as fam
import field_build_reference as ref
from beluga_amd import synth
from oracle import binding as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F, T = 0, 100
NARROW = ref.Params(2.0, 20.0, 0.5, 0.5, 0.2)


def grid5(rows):
    return np.array(rows, dtype=np.int8).reshape(5, 5)


def to_likelihood(sq, sigma=0.2, z_hit=0.5, z_random=0.5, max_laser=2.0):
    return z_hit / (sigma * math.sqrt(2 * math.pi)) * math.exp(-sq / (2 * sigma * sigma)) + z_random / max_laser


def only_value(adm):
    """The field of a reference whose every cell has one admissible value."""
    assert np.all(np.isnan(adm.likelihood[1:])) and not np.any(np.isnan(adm.likelihood[0]))
    return adm.likelihood[0]


def test_reference_reproduces_the_reference_projects_field_pins():
    # test_likelihood_field_model_base.cpp:34-60
    cells = grid5([F, F, F, F, T, F, F, F, T, F, F, F, T, F, F, F, T, F, F, F, T, F, F, F, F])
    expected = [0.025, 0.025, 0.025, 0.069, 1.022, 0.025, 0.027, 0.069, 1.022, 0.069, 0.025, 0.069, 1.022, 0.069, 0.025,
                0.069, 1.022, 0.069, 0.027, 0.025, 1.022, 0.069, 0.025, 0.025, 0.025]
    np.testing.assert_allclose(only_value(ref.admissible(cells, 0.5, NARROW)).ravel(), expected, atol=0.003)
    # :62-150 thick walls, the four combinations of model_unknown_space / only_obstacle_boundaries
    cells = grid5([F, F, F, F, F, F, T, T, T, F, F, T, T, T, F, F, T, T, T, F, F, F, F, F, F])
    p = ref.Params(10.0, 2.0, 0.5, 0.5, 0.2)
    f = only_value(ref.admissible(cells, 1.0, p, False, False))
    assert f[2, 2] == pytest.approx(to_likelihood(0.0), abs=1e-6) and f[1, 1] == pytest.approx(to_likelihood(0.0), abs=1e-6)
    f = only_value(ref.admissible(cells, 1.0, p, False, True))
    assert f[0, 0] == pytest.approx(to_likelihood(2.0), abs=1e-6)
    assert f[2, 2] == pytest.approx(to_likelihood(1.0), abs=1e-6) and f[1, 1] == pytest.approx(to_likelihood(0.0), abs=1e-6)
    f = only_value(ref.admissible(cells, 1.0, p, True, False))
    assert f[2, 2] == pytest.approx(to_likelihood(0.0), abs=1e-6) and f[1, 1] == pytest.approx(to_likelihood(0.0), abs=1e-6)
    f = only_value(ref.admissible(cells, 1.0, p, True, True))
    assert f[2, 2] == pytest.approx(0.5, abs=1e-6) and f[1, 1] == pytest.approx(to_likelihood(0.0), abs=1e-6)
    # :152-201 hollow thick walls
    cells = np.array([F, F, F, F, F, F, F, F, T, T, T, T, T, F, F, T, T, T, T, T, F, F, T, T, F, T, T, F, F, T, T, T, T, T, F,
                      F, T, T, T, T, T, F, F, F, F, F, F, F, F], dtype=np.int8).reshape(7, 7)
    f = only_value(ref.admissible(cells, 1.0, p, False, True))
    assert f[3, 3] == pytest.approx(to_likelihood(1.0), abs=1e-6) and f[2, 2] == pytest.approx(to_likelihood(1.0), abs=1e-6)
    # test_lfm_with_unknown_space.cpp:34-137
    cells = grid5([-1, -1, -1, 100, 100, -1, 0, 0, 0, 100, -1, 0, 0, 0, 100, 100, 0, 0, 0, 100, 100, 100, 100, 100, 100])
    U = 1 / 20.0
    f = only_value(ref.admissible(cells, 0.5, NARROW, True, False))
    np.testing.assert_allclose(f.ravel(), [U, U, U, 1.022, 1.022, U, 0.025, 0.027, 0.069, 1.022, U, 0.027, 0.025, 0.069, 1.022,
                                           1.022, 0.069, 0.069, 0.069, 1.022, 1.022, 1.022, 1.022, 1.022, 1.022], atol=0.003)
    f = only_value(ref.admissible(cells, 0.5, NARROW, True, True))
    np.testing.assert_allclose(f.ravel(), [U, U, U, 1.022, U, U, 0.025, 0.027, 0.069, 1.022, U, 0.027, 0.025, 0.069, 1.022,
                                           1.022, 0.069, 0.069, 0.069, 1.022, U, 1.022, 1.022, 1.022, U], atol=0.003)
    cells = grid5([-1, -1, -1, 100, 100, -1, -1, -1, 0, 0, -1, -1, -1, 0, 0, -1, -1, -1, 0, 0, -1, -1, -1, 100, 100])
    U = 1 / 100.0
    f = only_value(ref.admissible(cells, 0.5, ref.Params(2.0, 100.0, 0.5, 0.5, 0.2), True, False))
    np.testing.assert_allclose(f.ravel(), [U, U, U, 1.002, 1.002, U, U, U, 0.049, 0.049, U, U, U, 0.005, 0.005, U, U, U, 0.049, 0.049,
                                           U, U, U, 1.002, 1.002], atol=0.003)


def test_window_minimum_is_the_brute_force_minimum():
    for k, (W, H, density) in enumerate([(23, 17, 0.03), (40, 9, 0.01), (1, 30, 0.1), (31, 1, 0.1), (12, 12, 0.5)]):
        seeds = np.random.default_rng(k).random((H, W)) < density
        seeds[H // 2, W // 3] = True
        cells2, _ = ref.nearest_seed_sets(seeds, 1.0, 10 ** 6)  # (no cap: the whole map is in reach)
        assert np.array_equal(cells2, ref.brute_force_cells2(seeds)), (W, H)
    none, members = ref.nearest_seed_sets(np.zeros((4, 6), dtype=bool), 1.0, 100)
    assert np.all(none == -1) and len(members) == 1 and np.all(np.isnan(members[0]))
    # a cap: n(c) only where a seed lies within it
    seeds = np.zeros((1, 20), dtype=bool)
    seeds[0, 0] = True
    cells2, _ = ref.nearest_seed_sets(seeds, 1.0, 49)
    assert list(cells2[0]) == [x * x for x in range(8)] + [-1] * 12


@pytest.mark.parametrize("resolution", [0.05, 0.0625, 0.3])
@pytest.mark.parametrize("flags", fam.FLAGS, ids=[fam.flag_name(*f) for f in fam.FLAGS])
def test_reference_equals_the_wavefront_bit_for_bit_where_the_wavefront_is_exact(resolution, flags):
    unknown, edges = flags
    p = fam.WIDE
    R = fam.reach(resolution, p)
    one = fam.grid_with(2 * R + 7, R + 9, [(R + 2, 4)])
    one[R, 0:5] = -1
    one[2, R:R + 3] = 50
    apart = 2 * R + 3  # single seeds farther apart than twice the cap: no cell below the cap has two candidates
    many = fam.grid_with(2 * apart + 9, apart + 9, [(3, 2), (3 + apart, 4), (5 + 2 * apart, 1), (4, 3 + apart), (8 + apart, 6 + apart)])
    many[7, 0:30] = -1
    for cells in (one, many):
        adm = ref.admissible(cells, resolution, p, unknown, edges)
        want = orc.make_likelihood_field(cells, resolution, tuple(p), unknown, edges)
        assert np.array_equal(only_value(adm).view(np.uint32), want.view(np.uint32))
        assert (adm.cells2 >= 0).sum() > 0.2 * cells.size  # (the map is not mostly beyond the cap)


def _never_smaller(cells, resolution, p, unknown, edges):
    adm = ref.admissible(cells, resolution, p, unknown, edges)
    wave = orc.make_likelihood_field(cells, resolution, tuple(p), unknown, edges)
    largest = np.nanmax(adm.likelihood, axis=0)
    assert np.all(largest >= wave), int((largest < wave).sum())
    # the wavefront is right at most cells: where it holds an admissible value it holds it exactly (same arithmetic on the host)
    exact = np.any(adm.likelihood == wave[None], axis=0)
    return float(exact.mean()), adm


def test_reference_is_never_the_smaller_likelihood_on_rooms_and_turtlebot3():
    cells = synth.make_rooms_map(160, 120, seed=42, n_rooms=6)
    for unknown, edges in fam.FLAGS:
        share, _ = _never_smaller(cells, 0.05, fam.WIDE, unknown, edges)
        assert share > 0.9
    z = np.load(os.path.join(GOLDEN, "turtlebot3_world_grid.npz"))
    share, adm = _never_smaller(z["cells"], float(z["resolution"]), fam.WIDE, True, False)
    assert 0.9 < share < 1.0  # (the wavefront does miss the nearest obstacle at some cells of this map: DESIGN.md section 9)
    # the squared distances this map holds below the cap (some hundreds), each told apart from the next by the wide parameters
    n = np.unique(adm.cells2[adm.cells2 >= 0])
    sq = (n * float(z["resolution"]) ** 2).astype(np.float32)
    sq = sq[sq < ref.cap_value(fam.WIDE)]
    lik = np.unique(ref.likelihood(sq, fam.WIDE))
    print("turtlebot3: distinct squared distances below the cap:", len(sq), "least separation:", int(np.min(ref.ulps_between(lik[1:], lik[:-1]))))
    assert len(sq) > 400 and len(lik) == len(sq) and int(np.min(ref.ulps_between(lik[1:], lik[:-1]))) >= fam.SEPARATION


ALL_CASES = [c for cs in fam.families().values() for c in cs]


@pytest.mark.parametrize("c", ALL_CASES, ids=[c.name for c in ALL_CASES])
def test_every_case_of_the_gpu_suite_can_see_what_it_checks(c):
    assert c.params in fam.PARAMETER_SETS.values() and c.params.sigma_hit != 0.2
    H, W = c.cells.shape
    got = ref.separation_ulps(c.params, c.resolution, W, H, c.unknown)
    assert got is not None and got >= fam.SEPARATION, got


def test_the_turtlebot3_comparison_can_see_what_it_checks_and_the_narrow_sigma_cannot():
    z = np.load(os.path.join(GOLDEN, "turtlebot3_world_grid.npz"))
    H, W = z["cells"].shape
    assert ref.separation_ulps(fam.WIDE, float(z["resolution"]), W, H, True) >= fam.SEPARATION
    assert ref.separation_ulps(ref.Params(2.0, 100.0, 0.5, 0.5, 0.2), float(z["resolution"]), W, H, True) < 1  # distances collapse
    # a wide sigma alone does not make the overlay visible: with max_laser_distance = 100 it IS the cap
    far_laser = ref.Params(2.0, 100.0, 0.5, 0.5, 1.0)
    assert ref.overlay_value(far_laser) == ref.cap_value(far_laser)
    assert ref.separation_ulps(far_laser, float(z["resolution"]), W, H, True) == 0
    assert ref.overlay_value(fam.WIDE) < ref.cap_value(fam.WIDE)


def test_tie_cases_hold_ties():
    by_name = {c.name: c for c in fam.tie_cases()}
    for name, c in by_name.items():
        adm = fam.admissible_of(c)
        sizes = (~np.isnan(adm.squared)).sum(axis=0)
        centres = [fam.THREE_CENTRE] if "three" in name else fam.TIE_CENTRES
        assert all(adm.cells2[y, x] == 25 for x, y in centres)
        dyadic = c.resolution in (0.0625, 0.25)
        if dyadic:
            assert sizes.max() == 1, name  # tied seeds give one value
        elif c.resolution == fam.TIE_RES:
            assert all(sizes[y, x] == 2 for x, y in centres), name  # tied seeds whose float32 distances differ in the last bit
        members = adm.squared[:, centres[0][1], centres[0][0]]
        members = members[~np.isnan(members)]
        want = min(25 * c.resolution ** 2, float(ref.cap_value(c.params)))
        assert np.all(np.abs(members.astype(np.float64) - want) <= want * 2.0 ** -23)


def test_check_field_accepts_one_step_and_refuses_two():
    c = fam.tie_cases()[0]
    adm = fam.admissible_of(c)
    field = adm.likelihood[0].copy()
    assert fam.check_field(field, adm, c.name) == field.size
    bits = field.view(np.int32)
    bits[41, 290] += 1
    assert fam.check_field(field, adm, c.name) == field.size
    lone = np.argwhere((~np.isnan(adm.squared)).sum(axis=0) == 1)[0]
    bits[lone[0], lone[1]] += 2
    with pytest.raises(AssertionError, match="1 of"):
        fam.check_field(field, adm, c.name)
