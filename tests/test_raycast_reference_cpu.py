"""tests/raycast_reference.py against the CPU oracle's ray_cast (pinned by the reference project's own raycasting vectors in
tests/test_oracle_golden.py), against tests/beam_reference.py on the engineered families, and against the wrong restatements of the walk.
No device."""
import math

import numpy as np
import pytest

import beam_families as fam
import beam_reference as ref
import raycast_reference as rc
from oracle import binding as orc

# which family is meant for each wrong restatement of the walk (tests/test_beam_reference_cpu.py KILLS, the walk's part)
MEANT_FOR = {"trip_ge": "slopes", "past_the_end": "slopes", "stop_early": "slopes", "modified": "slopes", "unknown_free": "obstacle_at_k",
             "truncate": "cell_boundaries", "divide": "cell_boundaries", "outside_hit": "borders_and_tiny_grids", "corners": "range_terms"}

CENTER = np.zeros((5, 5), dtype=np.int8)
CENTER[2, 2] = ref.OCCUPIED
ANGLES = [0.0, 0.3, math.pi / 4, math.pi / 2, 2.0, math.pi, -2.5, -math.pi / 2, -0.4, 1.1]


def small_grids():
    salted = fam.salt(23, 31, k=17)
    walls = np.zeros((9, 33), dtype=np.int8)
    walls[0, :] = walls[-1, :] = ref.OCCUPIED
    walls[:, 0] = ref.UNKNOWN
    rotated = fam.ROTATED
    inside = [fam.local_pose(rotated, x, y, th) for x, y, th in ((3.5, 4.5, 0.0), (15.2, 11.9, 1.0), (30.99, 22.01, -2.0), (0.0, 0.0, 0.5))]
    outside = [fam.local_pose(rotated, x, y, th) for x, y, th in ((-3.0, 5.0, 0.1), (40.0, 10.0, 3.0), (12.0, -0.5, 1.5), (12.0, 23.0, -1.5))]
    return [
        (CENTER, 0.5, fam.IDENTITY, [orc.se2(0.5, 0.0, 0.0), orc.se2(0.0, 1.0, 0.0), orc.se2(1.0, 1.0, 0.0), orc.se2(0.0, 0.0, math.pi / 2)], 5.0),
        (CENTER, 0.5, orc.se2(0.5, 0.0, -math.pi / 4), [orc.se2(0.5, 0.0, 0.0), orc.se2(1.2, 0.7, 2.0)], 5.0),  # a rotated origin
        (salted, fam.RES, rotated, inside, 1.3),
        (salted, fam.RES, rotated, outside, 2.0),  # sources outside the grid
        (walls, 0.1, fam.IDENTITY, [orc.se2(1.65, 0.45, 0.2), orc.se2(0.05, 0.85, -0.2)], 0.55),  # a reach shorter than the way to a wall
    ]


@pytest.mark.parametrize("k", range(5))
def test_ranges_are_the_oracles_bit_for_bit(k):
    cells, res, origin, poses, max_range = small_grids()[k]
    got = rc.cast_rays(cells, res, origin, poses, rc.bearings_of_angles(ANGLES), max_range)
    hits = 0
    for i, pose in enumerate(poses):
        for b, a in enumerate(ANGLES):
            want = orc.ray_cast(cells, res, origin, pose, max_range, a)
            if want is None:
                assert got["hit_cells"][i, b] == -1 and got["ranges"][i, b] == max_range, (k, i, a)
            else:
                assert got["hit_cells"][i, b] >= 0 and got["ranges"][i, b] == want, (k, i, a, got["ranges"][i, b], want)
                hits += 1
    assert hits >= 1 or k == 3, (k, hits)  # (the sources outside the grid hit nothing: the trace ends at its first cell)
    if k == 3:
        assert got["cells_visited"] == 0 and (got["hit_cells"] == -1).all()


@pytest.mark.parametrize("name", sorted(fam.FAMILIES))
def test_one_case_of_every_family_is_beam_reference(name):
    case = fam.FAMILIES[name]()[0]
    if name == "beam_counts":
        case = fam.prefix(case, 65)
    want = ref.reference(case)
    got = rc.of_case(case)
    W = case["cells"].shape[1]
    assert np.array_equal(got["ranges"], want["expected"])
    assert np.array_equal(got["hit_cells"] >= 0, want["has_hit"])
    assert np.array_equal(got["hit_cells"][want["has_hit"]], (want["hit"][..., 1] * W + want["hit"][..., 0])[want["has_hit"]])
    assert np.array_equal(got["visited"], want["visited"]) and got["cells_visited"] == want["steps"]


@pytest.mark.parametrize("mutant", rc.WALK_MUTANTS)
def test_every_wrong_walk_changes_an_output_on_its_family(mutant):
    changed = 0
    for case in fam.FAMILIES[MEANT_FOR[mutant]]():
        good, bad = rc.of_case(case), rc.of_case(case, mutant)
        changed += int(((good["ranges"] != bad["ranges"]) | (good["hit_cells"] != bad["hit_cells"]) | (good["visited"] != bad["visited"])).sum())
        if changed:
            break
    assert changed >= 1, mutant


def test_the_walk_mutants_are_all_of_beam_references_but_the_mixtures():
    assert set(rc.WALK_MUTANTS) == set(ref.MUTANTS) - {"short_le", "tie_sqrt"} and set(MEANT_FOR) == set(rc.WALK_MUTANTS)


def test_out_of_reach_rays_hit_nothing_and_visit_nothing():
    cells = fam.salt(23, 31, k=17)
    res = 0.0625
    bearings = rc.bearings_of_angles(ANGLES)
    far = [[1.0, 0.0, 1e12, 0.0], [1.0, 0.0, 2.0 ** 30 * res, 0.5], [1.0, 0.0, 0.5, -(2.0 ** 30) * res], [0.0, 1.0, -1e12, 1e12]]
    got = rc.cast_rays(cells, res, fam.IDENTITY, far, bearings, 3.0)
    assert (got["ranges"] == 3.0).all() and (got["hit_cells"] == -1).all() and got["cells_visited"] == 0
    # one cell inside the bound is walked as the rule says: outside the grid, so nothing either - the two agree
    near = [[1.0, 0.0, (2.0 ** 30 - 1) * res, 0.5]]
    got = rc.cast_rays(cells, res, fam.IDENTITY, near, bearings, 3.0)
    assert (got["ranges"] == 3.0).all() and got["cells_visited"] == 0
    # a bearing that is no unit vector: a span of 2^27 cells is out of reach, whatever lies on the line
    long = rc.cast_rays(cells, res, fam.IDENTITY, [[1.0, 0.0, 0.5, 0.5]], [[2.0 ** 27, 0.0], [1.0, 0.0]], res)
    assert long["hit_cells"][0, 0] == -1 and long["visited"][0, 0] == 0 and long["visited"][0, 1] >= 1


def test_chunk_plan_covers_every_ray_once():
    for n, B, chunk in ((3, 129, 64), (65, 7, 100), (1, 4097, 4096), (5, 1, 64)):
        plan = rc.chunk_plan(n, B, chunk)
        assert [p[0] for p in plan] == list(range(0, n * B, max(chunk, 64))) and sum(p[1] for p in plan) == n * B
        for first, count, pose, bearing, poses, blocks in plan:
            assert pose * B + bearing == first and (first + count - 1) // B == pose + poses - 1 and blocks == -(-count // 256)
