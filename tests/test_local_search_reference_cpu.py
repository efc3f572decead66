"""tests/local_search_reference.py checked against itself and against brute force, on the CPU: its best-of-lattice against a sort of
the four keys on random scores with forced ties, its ids, its exact sums, its uniform covariance; and, with tests/lf_reference.py, that
the tie scenario of tests/test_gpu_local_search.py does give equal scores under the likelihood-field reference."""
import math
from fractions import Fraction

import numpy as np

import lf_reference
import local_search_reference as ref


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_best_of_agrees_with_a_brute_force_sort():
    rng = np.random.default_rng(1)
    for Kx, Kt in ((0, 0), (1, 1), (2, 3), (3, 0), (0, 4), (6, 8)):
        L = ref.candidates(Kx, Kt)
        for trial in range(12):
            palette = rng.uniform(0.1, 2.0, 1 + trial % 4)  # 1 .. 4 distinct scores: ties at every level
            scores = rng.choice(palette, L)
            if trial % 3 == 0:
                scores[rng.integers(0, L)] = np.nextafter(palette.max(), 3.0)  # a lone winner by one ulp
            rows = []
            for ident, s in enumerate(scores):
                i, j, k = ref.offsets_of(Kx, Kt, ident)
                rows.append((-ref.score_key(s), i * i + j * j, abs(k), ident))
            rows.sort()
            best, plateau = ref.best_of(scores, Kx, Kt)
            assert best == rows[0][3] and plateau == sum(1 for r in rows if r[0] == rows[0][0]) == int(np.count_nonzero(scores == scores[best]))
    # a plateau over the whole lattice: the centre
    for Kx, Kt in ((0, 0), (1, 1), (2, 3), (6, 8)):
        L = ref.candidates(Kx, Kt)
        assert ref.best_of(np.full(L, 0.37), Kx, Kt) == (ref.local_id(Kx, Kt, 0, 0, 0), L)
    # ties between the two signs of an offset go to the lower id: the negative one
    scores = np.zeros(ref.candidates(1, 1))
    scores[[ref.local_id(1, 1, 1, 0, 0), ref.local_id(1, 1, -1, 0, 0), ref.local_id(1, 1, 0, 1, 0)]] = 1.0
    assert ref.best_of(scores, 1, 1) == (ref.local_id(1, 1, -1, 0, 0), 3)
    scores[:] = 0.0
    scores[[ref.local_id(1, 1, 1, 1, 0), ref.local_id(1, 1, 0, 1, 1), ref.local_id(1, 1, 0, 1, -1)]] = 1.0
    assert ref.best_of(scores, 1, 1) == (ref.local_id(1, 1, 0, 1, -1), 3)


def test_score_key_orders_like_the_scores():
    values = [-math.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1.0000000000000002, 1e300, math.inf]
    keys = [ref.score_key(v) for v in values]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and ref.score_key(math.nan) == 0 < keys[0]


def test_ids_poses_and_plan():
    for Kx, Kt in ((0, 0), (1, 1), (2, 3), (32, 64)):
        L = ref.candidates(Kx, Kt)
        i, j, k = ref.offsets_of(Kx, Kt, np.arange(L))
        assert np.array_equal(ref.local_id(Kx, Kt, i, j, k), np.arange(L))
        assert i.min() == -Kx and i.max() == Kx and k.min() == -Kt and k.max() == Kt
    seed = np.array([math.cos(0.3) * (1 + 2.0 ** -51), math.sin(0.3) * (1 + 2.0 ** -51), 1.5, -2.5])
    poses = ref.lattice_poses(seed, 2, 3, 0.0125, math.pi / 360)
    assert np.array_equal(bits(poses[ref.local_id(2, 3, 0, 0, 0)]), bits(seed))
    assert np.all(np.abs(np.hypot(poses[:, 0], poses[:, 1]) - 1.0) < 1e-15)
    theta = np.arctan2(poses[:, 1], poses[:, 0]) - 0.3
    i, j, k = ref.offsets_of(2, 3, np.arange(len(poses)))
    assert np.allclose(theta, k * math.pi / 360, atol=1e-15) and np.allclose(poses[:, 2], 1.5 + i * 0.0125, atol=1e-15)
    assert ref.pass_plan(5, 27, 64) == (2, 54, 3) and ref.pass_plan(5, 175, 64) == (1, 175, 5) and ref.pass_plan(5, 1, 64) == (64, 64, 1)
    assert ref.pass_plan(2, 545025, 64) == (1, 545025, 2)


def test_exact_sums_and_the_uniform_covariance():
    rng = np.random.default_rng(4)
    for Kx, Kt in ((1, 1), (2, 3), (4, 5)):
        L = ref.candidates(Kx, Kt)
        scores = rng.uniform(0, 1, L)
        sums, magnitudes = ref.exact_sums(scores, Kx, Kt)
        i, j, k = ref.offsets_of(Kx, Kt, np.arange(L))
        assert sums[0] == sum(Fraction(float(s)) for s in scores) and sums[5] == sum(Fraction(float(s)) * int(a * b) for s, a, b in zip(scores, i, j))
        assert all(m >= abs(s) for s, m in zip(sums, magnitudes)) and magnitudes[0] == sums[0]
        uniform, _ = ref.exact_sums(np.ones(L), Kx, Kt)
        mean, cov = ref.finish_exact(uniform, 0.0125, math.pi / 360)
        assert mean == [0, 0, 0]
        assert cov[0][0] == cov[1][1] == ref.uniform_covariance(Kx, 0.0125) and cov[2][2] == ref.uniform_covariance(Kt, math.pi / 360)
        assert all(cov[a][b] == 0 for a in range(3) for b in range(3) if a != b)
    assert ref.uniform_covariance(1, 1.0) == Fraction(2, 3) and ref.uniform_covariance(0, 1.0) == 0


def test_the_gpu_tests_tie_scenario_ties_under_the_likelihood_field_reference():
    """The map, seed and scan of test_a_plateau_gives_the_centre_and_the_uniform_covariance (tests/test_gpu_local_search.py): every
    end-point of every pose of the widest lattice used there has a cell further than max_obstacle_distance (0.5 m) from every occupied
    cell, by brute force; on a field that is constant over such cells tests/lf_reference.py's weights are then equal, bit for bit."""
    W, H, resolution, max_obstacle_distance = 64, 48, 0.1, 0.5
    cells = np.zeros((H, W), dtype=np.int8)
    cells[0, :] = cells[-1, :] = cells[:, 0] = cells[:, -1] = 100
    cells[30, [x for x in range(W) if x < 12 or x > 18]] = 100
    cells[:30, 40] = 100
    origin = np.array([1.0, 0.0, -1.0, -1.0])
    seed = np.array([math.cos(0.3), math.sin(0.3), 1.05, 0.55])
    scan = np.array([[0.3, 0.0], [0.0, 0.3], [-0.3, 0.0], [0.2, -0.2]])
    poses = ref.lattice_poses(seed, 6, 8, 0.25 * resolution, math.pi / 360)
    xi, yi, inside = lf_reference.cells(cells.shape, resolution, origin, poses, scan)
    assert inside.all()
    oy, ox = np.nonzero(cells != 0)
    used = np.unique(np.stack([xi.ravel(), yi.ravel()], axis=1), axis=0)
    distance = np.sqrt(((used[:, 0, None] - ox) ** 2 + (used[:, 1, None] - oy) ** 2).min(axis=-1)) * resolution
    assert distance.min() > max_obstacle_distance + 2 * resolution
    y, x = np.mgrid[0:H, 0:W]
    everywhere = np.sqrt(((x[..., None] - ox) ** 2 + (y[..., None] - oy) ** 2).min(axis=-1)) * resolution
    field = np.where(everywhere >= max_obstacle_distance, 0.3, 0.3 + everywhere).astype(np.float32)
    weights = lf_reference.weights(field, resolution, origin, 100.0, poses, scan)
    assert np.all(bits(weights) == bits(weights[0]))
    assert len(np.unique(lf_reference.weights(field, resolution, origin, 100.0, poses + np.array([0.0, 0.0, 1.2, 0.0]), scan))) > 1  # (near a wall they differ)
