"""mcl_estimate_clusters and mcl_cluster_labels on the GPU, through the C ABI: every cluster of more than one particle
(beluga::estimate_clusters, algorithm/cluster_based_estimation.hpp:337-399) and the cluster id of every particle
(ParticleClusterizer::operator(), :269-304), against the CPU oracle on the set read back from the device.

What is expected is built the same way for every case: ids = orc.cluster_ids(states, w, *params); for each id with more than one
particle orc.estimate() over its particles and the numpy sum of their weights; the entries by descending weight, ties by ascending
id.  Tolerances are the project's: estimates 1e-9, weights 1e-12 relative, ids, counts, order and num_clusters exact.

Interleaved blobs: seed 7 (numpy PCG64).  For it the oracle finds 41 clusters of more than one particle in the interleaved arrangement
and 37 in the contiguous one (checked on the CPU when the seed was chosen; at least three are asserted below), and every full wave of
the interleaved set holds at least 10 different clusters.

Inside a filter: the second context is a landmark context (simpler to set up than an NDT one: a map of two landmarks, no grid)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from beluga_amd import capi, synth
from beluga_amd.amcl import (Amcl, AmclParams, DifferentialDriveModelParam, LandmarkMap, LandmarkMapBoundaries, LandmarkModelParam,
                             LandmarkPositionDetection, LikelihoodFieldModelParam, OccupancyGrid, se2_from_xytheta)
from oracle import binding as orc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
LF = LikelihoodFieldModelParam(max_obstacle_distance=2.0, max_laser_distance=100.0, z_hit=0.5, z_random=0.5, sigma_hit=0.2,
                               model_unknown_space=True)
DEFAULTS = (0.20, 0.524, 0.90)
COARSE = (1.0, math.pi / 2.0, 0.9)
SENTINEL = 0xA5A5A5A5


def _multicluster(xmin, xmax, ymin, ymax, step):  # test_cluster_based_estimation.cpp:67-94, as test_gpu_parity.py states it
    xw, yw = xmax - xmin, ymax - ymin
    xs = np.arange(step / 2.0, xw + 1e-12, step)
    ys = np.arange(step / 2.0, yw + 1e-12, step)
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    k = (2 * X >= xw) * 1.0 + (2 * Y >= yw) * 2.0 + 1.0
    wt = np.abs(np.sin(2.0 * np.pi * X / xw)) * np.abs(np.sin(2.0 * np.pi * Y / yw)) * k
    wt = np.maximum(0.0, wt - k / 2.0)
    states = np.stack([np.ones(X.size), np.zeros(X.size), X.ravel() + xmin, Y.ravel() + ymin], axis=1)
    return states, wt.ravel()


BLOBS = ((-4.0, -3.0, -2.0), (2.0, 1.0, 0.5), (6.0, -5.0, 2.5))
BLOB_SEED = 7


def _blobs(n, interleaved, centres=BLOBS, seed=BLOB_SEED):
    """Particle i from blob i mod B (every wave holds every cluster), or the blobs in B contiguous index ranges."""
    rng = np.random.Generator(np.random.PCG64(seed))
    blob = np.arange(n) % len(centres) if interleaved else np.arange(n) * len(centres) // n
    c = np.asarray(centres)[blob]
    x = c[:, 0] + rng.normal(0.0, 0.15, n)
    y = c[:, 1] + rng.normal(0.0, 0.15, n)
    t = c[:, 2] + rng.normal(0.0, 0.1, n)
    return np.stack([np.cos(t), np.sin(t), x, y], axis=1), rng.uniform(0.5, 1.5, n)


def _pairs():
    """80 pairs of identical poses 5 m apart on a line, pair k of weight 2^-(k mod 40) per particle (every sum is exact; pairs k and
    k + 40 tie), and five single particles, each heavier than any pair."""
    states, w = [], []
    for k in range(80):
        for _ in range(2):
            states.append(se2_from_xytheta(5.0 * k, 0.0, 0.0))
            w.append(2.0 ** -(k % 40))
    for j in range(5):
        states.append(se2_from_xytheta(5.0 * j, 50.0, 0.0))
        w.append(4.0)
    order = np.random.Generator(np.random.PCG64(5)).permutation(len(w))  # the two particles of a pair are not neighbours
    return np.array(states)[order], np.array(w)[order]


def _singles():  # NightmareDistributionTest (:388-415)
    far = np.array([se2_from_xytheta(-10, -10, 0), se2_from_xytheta(-10, 10, 0), se2_from_xytheta(10, -10, 0), se2_from_xytheta(10, 10, 0)])
    return far, np.full(4, 0.2)


SETS = {
    "four_peaks": (lambda: _multicluster(0.0, 36.0, 0.0, 36.0, 1.0), COARSE),            # 1296 particles
    "fine_multicluster": (lambda: _multicluster(-2.0, 2.0, -2.0, 2.0, 0.025), DEFAULTS),  # 25 600: several chunks
    "blobs_interleaved": (lambda: _blobs(70_001, True), DEFAULTS),                          # a partial last wave
    "blobs_contiguous": (lambda: _blobs(70_001, False), DEFAULTS),
    "pairs": (_pairs, DEFAULTS),
    "singles": (_singles, DEFAULTS),
}
WITH_CLUSTERS = ["four_peaks", "fine_multicluster", "blobs_interleaved", "blobs_contiguous"]


def _expected(states, w, res):
    ids = orc.cluster_ids(states, w, *res).astype(np.int64)
    counts = np.bincount(ids)
    entries = []
    for c in np.flatnonzero(counts > 1):
        sel = ids == c
        pose, cov = orc.estimate(states[sel], w[sel])
        entries.append((int(c), int(counts[c]), float(w[sel].sum()), pose, cov))
    entries.sort(key=lambda e: (-e[2], e[0]))
    return ids, entries


def _rooms_filter(n):
    cells = synth.make_rooms_map(64, 64, seed=1, n_rooms=12)
    grid = OccupancyGrid(cells=cells, resolution=0.05, origin=se2_from_xytheta(-1.6, -1.6, 0.0))
    return Amcl(grid, MOTION, LF, AmclParams(min_particles=n, max_particles=n), seed=11)


def _call(f, res, capacity=capi.MCL_MAX_CLUSTER_ESTIMATES, null_out=False):
    """mcl_estimate_clusters through the C ABI: (status, num_clusters, the whole out array)."""
    cp = capi.ClusterParams(*res)
    out = (capi.ClusterEstimate * max(capacity, 1))()
    for e in out:
        e.id = SENTINEL
    total = C.c_uint64(SENTINEL)
    st = f._lib.mcl_estimate_clusters(f._ctx, C.byref(cp), None if null_out else out, capacity, C.byref(total))
    return st, total.value, out


def _labels(f, res):
    cp = capi.ClusterParams(*res)
    labels = np.full(f.num_particles(), SENTINEL, dtype=np.uint32)
    assert f._lib.mcl_cluster_labels(f._ctx, C.byref(cp), labels.ctypes.data_as(capi.c_u32_p)) == capi.MCL_OK
    return labels


def _check_entries(out, want):
    for k, (cid, count, weight, pose, cov) in enumerate(want):
        e = out[k]
        print(f"entry {k}: id {e.id} (want {cid}) count {e.count} (want {count}) weight {e.weight!r} (want {weight!r}) "
              f"pose err {np.abs(np.array(e.estimate.pose) - pose).max():.3e} "
              f"cov err {np.abs(np.array(e.estimate.covariance).reshape(3, 3) - cov).max():.3e}")
        assert (e.id, e.count) == (cid, count), k
        assert e.weight == pytest.approx(weight, rel=1e-12, abs=0), k
        np.testing.assert_allclose(np.array(e.estimate.pose), pose, rtol=0, atol=1e-9, err_msg=f"entry {k}")
        np.testing.assert_allclose(np.array(e.estimate.covariance).reshape(3, 3), cov, rtol=0, atol=1e-9, err_msg=f"entry {k}")
    for e in out[len(want):]:
        assert e.id == SENTINEL  # nothing is written beyond the entries


class Loaded:
    """A set on an LF context, read back, and what the oracle expects of it; shared by the tests (nothing modifies the set)."""

    def __init__(self, name):
        make, self.res = SETS[name]
        states, w = make()
        self.f = _rooms_filter(len(w))
        self.f.set_particles(states, w)
        self.states, self.w = self.f.particles()
        assert np.array_equal(self.states, states) and np.array_equal(self.w, w)
        self.ids, self.want = _expected(self.states, self.w, self.res)


@pytest.fixture(scope="module")
def loaded():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Loaded(name)
        return cache[name]
    yield get
    for s in cache.values():
        s.f.close()


@pytest.mark.parametrize("name", WITH_CLUSTERS)
def test_every_cluster_matches_the_oracle(loaded, name):
    s = loaded(name)
    if name.startswith("blobs"):
        assert len(s.want) >= 3  # (seed 7: checked on the CPU when the seed was chosen)
        if name == "blobs_interleaved":  # every wave holds every cluster
            blocks = s.ids[:70_001 - 70_001 % 64].reshape(-1, 64)
            assert min(len(np.unique(b)) for b in blocks) >= 3
    st, total, out = _call(s.f, s.res)
    assert st == capi.MCL_OK
    assert total == len(s.want) <= capi.MCL_MAX_CLUSTER_ESTIMATES
    _check_entries(out, s.want)
    if name == "four_peaks":  # ClusterStateEstimationStep (:291-315): four clusters, by ascending weight at these means
        assert total == 4
        for e, (x, y) in zip(reversed(out[:4]), [(9.0, 9.0), (27.0, 9.0), (9.0, 27.0), (27.0, 27.0)]):
            np.testing.assert_allclose(np.array(e.estimate.pose), [1.0, 0.0, x, y], atol=1e-6)


def test_more_clusters_than_the_cap(loaded):
    s = loaded("pairs")
    assert len(s.want) == 80 and all(count == 2 for _, count, _, _, _ in s.want)
    st, total, out = _call(s.f, s.res)
    assert st == capi.MCL_OK and total == 80
    _check_entries(out, s.want[:64])
    weights = [e.weight for e in out]
    assert weights == [2.0 * 2.0 ** -(k // 2) for k in range(64)]  # exact sums: pairs k and k + 40 tie
    for k in range(0, 64, 2):
        assert out[k].id < out[k + 1].id  # ties in ascending id
    st, total, few = _call(s.f, s.res, capacity=3)
    assert st == capi.MCL_OK and total == 80
    _check_entries(few, s.want[:3])
    st, total, untouched = _call(s.f, s.res, capacity=0, null_out=True)
    assert st == capi.MCL_OK and total == 80 and untouched[0].id == SENTINEL


def test_no_cluster_of_more_than_one_particle(loaded):
    s = loaded("singles")
    assert s.want == []
    st, total, out = _call(s.f, s.res)
    assert st == capi.MCL_OK and total == 0
    assert out[0].id == SENTINEL  # nothing written; the overall estimate stays mcl_cluster_based_estimate's answer
    pose, cov = s.f.cluster_based_estimate(*s.res)
    want_pose, want_cov = orc.estimate(s.states, s.w)
    np.testing.assert_allclose(pose, want_pose, atol=1e-9)
    np.testing.assert_allclose(cov, want_cov, atol=1e-9)


@pytest.mark.parametrize("name", sorted(SETS))
def test_labels_are_the_clusterizers(loaded, name):
    s = loaded(name)
    labels = _labels(s.f, s.res)
    assert np.array_equal(labels.astype(np.int64), s.ids)


@pytest.mark.parametrize("name", WITH_CLUSTERS)
def test_first_entry_is_cluster_based_estimate(loaded, name):
    s = loaded(name)
    st, _, out = _call(s.f, s.res, capacity=1)
    assert st == capi.MCL_OK
    pose, cov = s.f.cluster_based_estimate(*s.res)
    np.testing.assert_allclose(np.array(out[0].estimate.pose), pose, rtol=0, atol=1e-9)
    np.testing.assert_allclose(np.array(out[0].estimate.covariance).reshape(3, 3), cov, rtol=0, atol=1e-9)


@pytest.mark.parametrize("name", ["blobs_interleaved", "blobs_contiguous"])
def test_two_calls_return_the_same_bits(loaded, name):
    s = loaded(name)
    _, total_a, a = _call(s.f, s.res)
    _, total_b, b = _call(s.f, s.res)
    assert total_a == total_b >= 3
    assert bytes(a) == bytes(b)


def test_facade_returns_the_same_entries(loaded):
    s = loaded("fine_multicluster")
    total, found = s.f.estimate_clusters(*s.res, max_clusters=2)
    assert total == 4 and len(found) == 2
    for (cid, count, weight, pose, cov), want in zip(found, s.want):
        assert (cid, count) == want[:2] and weight == pytest.approx(want[2], rel=1e-12)
        np.testing.assert_allclose(pose, want[3], atol=1e-9)
        np.testing.assert_allclose(cov, want[4], atol=1e-9)
    assert np.array_equal(s.f.cluster_labels(*s.res).astype(np.int64), s.ids)


def test_errors():
    f = _rooms_filter(100)
    lib = f._lib
    total = C.c_uint64(0)
    out = (capi.ClusterEstimate * 4)()
    labels = np.zeros(100, dtype=np.uint32)
    assert lib.mcl_estimate_clusters(f._ctx, None, out, 4, C.byref(total)) == capi.MCL_ERR_NOT_READY  # no particles
    assert lib.mcl_cluster_labels(f._ctx, None, labels.ctypes.data_as(capi.c_u32_p)) == capi.MCL_ERR_NOT_READY
    f.initialize((0.0, 0.0, 0.0), np.diag([0.01, 0.01, 0.01]))
    for bad in ((0.0, 0.524, 0.9), (0.2, -1.0, 0.9), (0.2, 0.524, 1.0), (0.2, 0.524, -0.1)):
        cp = capi.ClusterParams(*bad)
        assert lib.mcl_estimate_clusters(f._ctx, C.byref(cp), out, 4, C.byref(total)) == capi.MCL_ERR_INVALID_ARGUMENT
        assert lib.mcl_cluster_labels(f._ctx, C.byref(cp), labels.ctypes.data_as(capi.c_u32_p)) == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.mcl_estimate_clusters(f._ctx, None, None, 4, C.byref(total)) == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.mcl_estimate_clusters(f._ctx, None, out, 4, None) == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.mcl_cluster_labels(f._ctx, None, None) == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.mcl_estimate_clusters(f._ctx, None, out, 4, C.byref(total)) == capi.MCL_OK  # NULL parameters: the defaults
    assert total.value >= 1
    f.close()


# ---- inside a filter ----------------------------------------------------------------------------------------------------------------
TWO_POSES = ((-2.0, -0.5, 0.0), (2.0, 0.5, math.pi))  # the turtlebot world is symmetric enough for both to be free


def _two_blobs(n):
    return _blobs(n, False, centres=TWO_POSES, seed=9)


def _check_against_read_back(f, res=DEFAULTS):
    states, w = f.particles()
    ids, want = _expected(states, w, res)
    assert len(want) >= 2
    st, total, out = _call(f, res)
    assert st == capi.MCL_OK and total == len(want)
    _check_entries(out, want[:capi.MCL_MAX_CLUSTER_ESTIMATES])
    assert np.array_equal(_labels(f, res).astype(np.int64), ids)
    return w


def test_inside_a_likelihood_field_filter():
    """5000 particles around two poses on the turtlebot grid, two mcl_update cycles without resampling (resample_interval 100): the
    weights the sensor model left and the set in the order the cycle keeps it are the input."""
    z = np.load(os.path.join(GOLDEN, "turtlebot3_world_grid.npz"))
    ox, oy, ot = z["origin_xytheta"]
    grid = OccupancyGrid(cells=z["cells"], resolution=float(z["resolution"]), origin=se2_from_xytheta(ox, oy, ot))
    n = 5000
    f = Amcl(grid, MOTION, LF, AmclParams(min_particles=n, max_particles=n, resample_interval=100), seed=11)
    states, _ = _two_blobs(n)
    f.set_particles(states, np.ones(n))
    angles = synth.lidar_angles(90, 270.0)
    pose, odom = TWO_POSES[0], (0.0, 0.0, 0.0)
    for c in range(2):
        pose = synth.odometry_step(pose, 0.3, 0.05)
        odom = synth.odometry_step(odom, 0.3, 0.05)
        ranges = synth.cast_scan(grid.cells, grid.resolution, (grid.origin[2], grid.origin[3]), pose, angles, 8.0, 0.01, c)
        assert f.update(se2_from_xytheta(*odom), synth.scan_points(ranges, angles)) is not None
        assert not f.last_info["resampled"]
    w = _check_against_read_back(f)
    assert len(np.unique(w)) > n // 2  # the weights are the sensor model's, not units
    f.close()


def test_on_a_landmark_context():
    """The same two-blob set on a landmark context (the sensor kind that is simplest to set up without a grid): the clustering reads
    the particle set alone, whatever the sensor model."""
    lmap = LandmarkMap(LandmarkMapBoundaries((-10.0, -10.0, 0.0), (10.0, 10.0, 2.0)),
                       [LandmarkPositionDetection((1.0, 2.0, 1.0), 0), LandmarkPositionDetection((-3.0, 0.5, 0.5), 1)])
    n = 5000
    f = Amcl(lmap, MOTION, LandmarkModelParam(sigma_range=0.4, sigma_bearing=0.15, random_prob=1e-3),
             AmclParams(min_particles=n, max_particles=n), seed=11)
    states, w = _two_blobs(n)
    f.set_particles(states, w)
    _check_against_read_back(f)
    f.close()
