"""The 2D NDT sensor model on the GPU (ndt_kernels.hip through the C ABI) against the numpy restatement of the reference
(tests/ndt_reference.py) and the CPU oracle's cycle stages.  Tolerances as in test_gpu_parity.py: weights relative 1e-12,
resampling counts and KLD cut bit-exact, ancestors except at CDF-step ties, estimates 1e-9.

These tests draw random poses and scans: they cover real maps through the measurement fit, every kernel shape, large n (to 1M
particles) and whole cycles, but a random pose never puts a transformed mean on a cell edge.  The cell CHOICE - edges, the centre box,
the ends of int32, singular sums - is held by tests/test_gpu_ndt_edges.py against ndt_reference.weights_exact, with a derived tolerance."""
import math
import os
import subprocess

import numpy as np
import pytest

from beluga_amd import capi, synth
from beluga_amd.amcl import (Amcl, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam, NDTMap2d, NDTModelParam2d,
                             OccupancyGrid, load_ndt_map_npz, ndt_measurement_cells, se2_from_xytheta)
from oracle import binding as orc

import ndt_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
MOTION_T = (0.1, 0.05, 0.1, 0.05)
NODE = NDTModelParam2d(minimum_likelihood=0.01, d1=1.0, d2=0.6)
CROSS = ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1))
HASH = (0.5, 0.5, math.radians(10))


def turtlebot_ndt():
    return load_ndt_map_npz(os.path.join(GOLDEN, "turtlebot3_world_ndt.npz"))


def turtlebot_grid():
    z = np.load(os.path.join(GOLDEN, "turtlebot3_world_grid.npz"))
    ox, oy, ot = z["origin_xytheta"]
    return OccupancyGrid(cells=z["cells"], resolution=float(z["resolution"]), origin=se2_from_xytheta(ox, oy, ot))


def synthetic_ndt(size=240, res=0.05, ndt_res=0.5, seed=3):
    """A rooms map centred on the origin (keys on both sides of zero) and its NDT fit."""
    cells = synth.make_rooms_map(size, size, seed=seed, n_rooms=6)
    origin = (-size * res / 2, -size * res / 2)
    keys, means, covs = synth.make_ndt_map(cells, res, ndt_res, origin_xy=origin, seed=seed)
    return NDTMap2d(keys, means, covs, ndt_res), cells, origin


def ref_map(m):
    return ref.NdtMap(m.cells, m.means, m.covariances, m.resolution)


def new_ndt(ndt_map, n, sensor=NODE, **kw):
    params = AmclParams(min_particles=kw.pop("min_particles", n), max_particles=n, **kw)
    return Amcl(ndt_map, MOTION, sensor, params, seed=kw.pop("seed", 11))


def ring_scan(center, n=360, radius=(1.0, 3.5), seed=0):
    """Points around the robot at ranges that vary smoothly with the bearing (cells of >= 5 points in most directions)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    a = np.linspace(-math.pi, math.pi, n, endpoint=False)
    r = radius[0] + (radius[1] - radius[0]) * (0.5 + 0.5 * np.sin(3 * a)) + rng.normal(0, 0.01, n)
    return np.stack([r * np.cos(a), r * np.sin(a)], 1) + np.asarray(center)


def test_reference_likelihood_vectors_through_the_device_kernel():
    m = NDTMap2d(np.array([[0, 0], [1, 1]], dtype=np.int32), np.array([[0.5, 0.5], [1.5, 1.5]]),
                 np.array([np.diag([0.5, 0.3]), np.diag([0.5, 0.5])]), 1.0)
    f = new_ndt(m, 1, NDTModelParam2d(minimum_likelihood=1e-6))
    want = [((0.5, 0.5), 1.3678794411714423), ((0.8, 0.5), 1.4307317817730123), ((0.5, 0.8), 1.4200370805919718),
            ((1.5, 1.5), 1.3246524673583497), ((1.8, 1.5), 1.1859229670198237), ((1.5, 1.8), 1.1669230426687498)]
    for mean, value in want:
        f.set_particles(np.array([[1.0, 0.0, 0.0, 0.0]]), np.ones(1))
        f.reweight_ndt_cells(np.array([mean]), np.diag([0.5, 0.5]).reshape(1, 4))
        assert f.particles()[1][0] == pytest.approx(1.0 + value, rel=1e-14)
    f.close()


def test_reference_sensor_model_vector_through_mcl_reweight():
    pts = np.array([(0.1, 0.2), (0.112, 0.22), (0.15, 0.23), (0.1, 0.24), (0.16, 0.25), (0.1, 0.26)])
    means, covs = ref.to_cells(pts, 0.5)
    keys = np.array([[int(mm[0] / 0.5), int(mm[1] / 0.5)] for mm in means], dtype=np.int32)
    f = new_ndt(NDTMap2d(keys, means, covs, 0.5), 3, NDTModelParam2d())
    f.set_particles(np.array([se2_from_xytheta(0, 0, 0), se2_from_xytheta(-10, -10, 0), se2_from_xytheta(0.1, 0.1, 0)]), np.ones(3))
    f.reweight(pts)
    w = f.particles()[1]
    assert w[0] == 2.0 and w[1] == 1.0 and w[2] > 1.0
    f.close()


CASES = [("turtlebot", NODE), ("turtlebot", NDTModelParam2d(0.0, 1.0, 1.0)), ("synthetic", NODE),
         ("synthetic", NDTModelParam2d(0.0, 1.0, 0.6, ((0, 0),))), ("synthetic", NDTModelParam2d(0.01, 1.0, 0.6, CROSS)),
         # reach 2 and 3: the index grid's border of 2 x reach and the centre-box test beyond one cell
         ("synthetic", NDTModelParam2d(0.01, 1.0, 0.6, ((0, 0), (2, 0), (-2, 0), (0, 3), (-1, -3)))),
         ("turtlebot", NDTModelParam2d(0.0, 1.0, 0.6, ((-2, 0), (2, 0), (0, -2), (0, 2), (0, 0))))]


@pytest.mark.parametrize("which,sensor", CASES)
@pytest.mark.parametrize("n", [1, 63, 64, 1000, 100_000])
def test_reweight_matches_the_restatement(which, sensor, n):
    if which == "turtlebot":
        m = turtlebot_ndt()
        center, spread = (0.0, 0.0), (1.2, 1.2, 3.0)
    else:
        m = synthetic_ndt()[0]
        center, spread = (0.0, 0.0), (3.0, 3.0, 3.0)
    states = synth.normal_particles(n, (center[0], center[1], 0.0), spread, seed=n)
    w0 = np.random.Generator(np.random.PCG64(n)).uniform(0.5, 2.0, n)
    pts = ring_scan(center, 720, seed=n % 7)
    f = new_ndt(m, n, sensor)
    f.set_particles(states, w0)
    f.reweight(pts)
    got = f.particles()[1]
    means, covs = ref.to_cells(pts, m.resolution)
    assert len(means) > 10
    want = w0 * ref.weights_vectorized(ref_map(m), states, means, covs, sensor.minimum_likelihood, sensor.d1, sensor.d2,
                                       sensor.neighbors_kernel)
    np.testing.assert_allclose(got, want, rtol=1e-12)
    if n >= 1000:  # (and the map is actually hit)
        assert np.mean(want > w0 * (1.0 + len(means) * sensor.minimum_likelihood) * (1 + 1e-12)) > 0.01
    f.close()


def test_reweight_1m_sampled_against_the_restatement():
    m = turtlebot_ndt()
    n = 1_000_000
    states = synth.normal_particles(n, (0.0, 0.0, 0.0), (1.5, 1.5, 3.0), seed=5)
    pts = ring_scan((0.0, 0.0), 1080, seed=2)
    f = new_ndt(m, n)
    f.set_particles(states, np.ones(n))
    f.reweight(pts)
    got = f.particles()[1]
    idx = np.random.Generator(np.random.PCG64(9)).choice(n, 20_000, replace=False)
    means, covs = ref.to_cells(pts, m.resolution)
    want = ref.weights_vectorized(ref_map(m), states[idx], means, covs, NODE.minimum_likelihood, NODE.d1, NODE.d2)
    np.testing.assert_allclose(got[idx], want, rtol=1e-12)
    f.close()


def test_device_measurement_cells_equal_the_host_fit():
    pts = ring_scan((0.3, -0.2), 720, seed=4)
    gm, gc = ndt_measurement_cells(pts, 1.0)
    m = turtlebot_ndt()
    f = new_ndt(m, 500)
    states = synth.normal_particles(500, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), seed=1)
    f.set_particles(states, np.ones(500))
    f.reweight(pts)
    a = f.particles()[1]
    f.set_particles(states, np.ones(500))
    f.reweight_ndt_cells(gm, gc.reshape(-1, 4))
    assert np.array_equal(a, f.particles()[1])
    f.close()


def _cycle_against_oracle(min_p, max_p, cycles=8, seed=21):
    m = turtlebot_ndt()
    rm = ref_map(m)
    # (recovery filters that never move apart: no random states in these cycles - test_recovery_injection_draws_from_the_estimate)
    params = AmclParams(min_particles=min_p, max_particles=max_p, alpha_slow=0.0, alpha_fast=0.0)
    gpu = Amcl(m, MOTION, NODE, params, seed=seed)
    truth = (-0.5, 0.3, 0.2)
    cov = np.diag([0.09, 0.09, 0.04])
    gpu.initialize(truth, cov)
    states, w = orc.init_normal(max_p, truth, cov, seed)
    g0, _ = gpu.particles()
    np.testing.assert_allclose(g0, states, rtol=1e-12, atol=1e-12)
    states = g0.copy()
    odom = (0.0, 0.0, 0.0)
    prev = None
    for c in range(cycles):
        odom = synth.odometry_step(odom, 0.3, 0.05)
        ctrl = se2_from_xytheta(*odom)
        pts = ring_scan((0.0, 0.0), 360, seed=c)
        gpu.force_update()
        est = gpu.update(ctrl, pts)
        assert est is not None
        # amcl_core.hpp:174-200 on the oracle's stages: propagate, reweight (restatement), normalize, resample, estimate
        sampler = orc.diffdrive_sampler(ctrl, prev if prev is not None else ctrl, MOTION_T)
        prev = ctrl
        states = orc.propagate(states, sampler, seed, c + 1)
        means, covs = ref.to_cells(pts, m.resolution)
        w = orc.normalize(w * ref.weights_vectorized(rm, states, means, covs, NODE.minimum_likelihood, NODE.d1, NODE.d2))[0]
        want, anc = orc.resample(states, w, min_p, max_p, 0.05, 3.0, HASH, 0.0, seed, c + 1)
        got, gw = gpu.particles()
        assert len(got) == len(want), f"cycle {c}: particle counts differ"
        assert np.all(gw == 1.0)
        flips = int(np.any(np.abs(got - want) > 1e-9, axis=1).sum())
        assert flips <= 3, f"cycle {c}: {flips} ancestors differ"
        om, oc = orc.estimate(got, np.ones(len(got)))
        np.testing.assert_allclose(est[0], om, atol=1e-9)
        np.testing.assert_allclose(est[1], oc, rtol=1e-8, atol=1e-9)
        states, w = got, np.ones(len(got))
    gpu.close()


def test_update_cycle_fixed_size_matches_the_oracle_stages():
    _cycle_against_oracle(20_000, 20_000)


def test_update_cycle_kld_matches_the_oracle_stages():
    _cycle_against_oracle(500, 50_000)


def _tie_flips(got, want, w, seed, step, rows):
    """Rows of `rows` where got and want differ by more than 1e-9 (the propagation's rounding: test_gpu_parity.py), all explained by a
    CDF step within 1e-9 of the draw."""
    cdf = np.cumsum(w / w.sum())
    diff = [j for j in rows if np.any(np.abs(got[j] - want[j]) > 1e-9)]
    for j in diff:
        r = orc.draw(seed, step, 2, int(j))
        u = float((int(r[0]) << 32 | int(r[1])) >> 11) * 2.0 ** -53
        k = np.searchsorted(cdf, u, side="left")
        near = min(abs(cdf[min(k, len(cdf) - 1)] - u), abs(cdf[max(k - 1, 0)] - u))
        assert near < 1e-9, f"slot {j}: differs from the oracle's ancestor away from a CDF step (gap {near})"
    return len(diff)


def test_recovery_injection_draws_from_the_estimate():
    """Stage-level resample with p = 0.6 on a BIMODAL set (two clusters 2 m apart): the slots the Bernoulli stream selects are the
    oracle's (random_intersperse), the other slots hold the oracle's ancestors, and the injected states follow N(estimate) - which puts
    most of them between the clusters, where no particle of the set is."""
    m = turtlebot_ndt()
    n = 200_000
    a = synth.normal_particles(n // 2, (-1.0, -0.3, 0.5), (0.05, 0.05, 0.05), seed=8)
    b = synth.normal_particles(n - n // 2, (1.0, -0.3, 0.5), (0.05, 0.05, 0.05), seed=9)
    states = np.concatenate([a, b])
    w = np.random.Generator(np.random.PCG64(2)).uniform(0.2, 1.0, n)
    wn = orc.normalize(w)[0]
    mean, cov = orc.estimate(states, wn)
    runs = []
    for _ in range(2):
        f = new_ndt(m, n)
        f.set_particles(states, w)
        f.normalize()
        assert f.resample(0.6, step=5) == n
        runs.append(f.particles()[0])
        f.close()
    assert np.array_equal(runs[0], runs[1])  # bitwise reproducible
    got = runs[0]
    want, anc = orc.resample(states, wn, n, n, 0.05, 3.0, HASH, 0.6, 11, 5, free_xy=np.zeros((1, 2)))
    inj = anc == -1
    assert inj.sum() > 100_000 and not inj[0]
    assert _tie_flips(got, want, wn, 11, 5, np.flatnonzero(~inj)) <= 5
    # injected: not states of the set, and distributed as N(estimate)
    between = np.mean(np.abs(got[inj, 2]) < 0.5)
    assert between > 0.3  # N(0, ~1): 38 % within 0.5 of the mean; the set has none there
    assert np.mean(np.abs(got[~inj, 2]) < 0.5) == 0.0
    th = np.arctan2(got[inj, 1], got[inj, 0])
    mt = math.atan2(mean[1], mean[0])
    xs = np.stack([got[inj, 2], got[inj, 3], np.angle(np.exp(1j * (th - mt))) + mt], 1)
    k = len(xs)
    mu = np.array([mean[2], mean[3], mt])
    sd = np.sqrt(np.diag(cov))
    assert np.all(np.abs(xs.mean(0) - mu) < 4 * sd / math.sqrt(k))
    emp = np.cov(xs.T)
    for i in range(3):  # variance of a sample variance of a normal: 2 s^4 / (k - 1)
        assert abs(emp[i, i] - cov[i, i]) < 4 * cov[i, i] * math.sqrt(2.0 / (k - 1))
    # kurtosis of x: 3 for the normal draws (the bimodal set's is ~1)
    zx = (xs[:, 0] - xs[:, 0].mean()) / xs[:, 0].std()
    assert abs(np.mean(zx ** 4) - 3.0) < 0.1


def test_update_cycle_with_injection_matches_the_oracle_stages():
    """mcl_update on an NDT context with 20 000 particles (10 chunks of the normalisation) and the recovery filters put apart: the cycle's
    random state probability, the injected slots and the other slots' ancestors follow the oracle's stages; the next cycle (filters
    reset, p = 0) as well."""
    m = turtlebot_ndt()
    rm = ref_map(m)
    n, seed = 20_000, 21
    a_slow, a_fast = 0.001, 0.1
    gpu = Amcl(m, MOTION, NODE, AmclParams(min_particles=n, max_particles=n, alpha_slow=a_slow, alpha_fast=a_fast), seed=seed)
    truth = (-0.5, 0.3, 0.2)
    cov = np.diag([0.09, 0.09, 0.04])
    gpu.initialize(truth, cov)
    states, w = gpu.particles()
    slow, fast = 2.0 / n, 0.5 / n
    gpu.debug_set_recovery_filters(slow, fast)
    odom, prev = (0.0, 0.0, 0.0), None
    injected = 0
    for c in range(3):
        odom = synth.odometry_step(odom, 0.3, 0.05)
        ctrl = se2_from_xytheta(*odom)
        pts = ring_scan((0.0, 0.0), 360, seed=c)
        gpu.force_update()
        est = gpu.update(ctrl, pts)
        assert est is not None
        sampler = orc.diffdrive_sampler(ctrl, prev if prev is not None else ctrl, MOTION_T)
        prev = ctrl
        states = orc.propagate(states, sampler, seed, c + 1)
        means, covs = ref.to_cells(pts, m.resolution)
        w = orc.normalize(w * ref.weights_vectorized(rm, states, means, covs, NODE.minimum_likelihood, NODE.d1, NODE.d2))[0]
        # ThrunRecoveryProbabilityEstimator (thrun_recovery_probability_estimator.hpp:69-89) on the normalised weights
        avg = w.sum() / len(w)
        slow = avg if slow == 0.0 else slow + a_slow * (avg - slow)
        fast = avg if fast == 0.0 else fast + a_fast * (avg - fast)
        p = min(max(1.0 - fast / slow, 0.0), 1.0) if slow != 0.0 else 0.0
        assert gpu.last_info["random_state_probability"] == pytest.approx(p, abs=1e-12), f"cycle {c}"
        p = gpu.last_info["random_state_probability"]  # (the library's own bits for the Bernoulli comparisons)
        if p > 0.0:
            slow = fast = 0.0
        want, anc = orc.resample(states, w, n, n, 0.05, 3.0, HASH, p, seed, c + 1, free_xy=np.zeros((1, 2)))
        got, gw = gpu.particles()
        assert len(got) == len(want) == n and np.all(gw == 1.0)
        inj = anc == -1
        injected += int(inj.sum())
        assert _tie_flips(got, want, w, seed, c + 1, np.flatnonzero(~inj)) <= 3, f"cycle {c}"
        if inj.any():  # the injected slots hold states of no ancestor: N(estimate of the normalised set)
            mean, ecov = orc.estimate(states, w)
            assert abs(got[inj, 2].mean() - mean[2]) < 5 * math.sqrt(ecov[0, 0] / inj.sum())
        om, oc = orc.estimate(got, np.ones(n))
        np.testing.assert_allclose(est[0], om, atol=1e-9)
        np.testing.assert_allclose(est[1], oc, rtol=1e-8, atol=1e-9)
        states, w = got, np.ones(n)
    assert injected > 1000
    gpu.close()


def test_rejected_covariance_leaves_the_set_unchanged():
    m = turtlebot_ndt()
    f = new_ndt(m, 64)
    states = np.tile(se2_from_xytheta(0.1, 0.2, 0.3), (64, 1))
    states[:, :2] = [[1.0, 0.0] if i % 2 else [-1.0, 0.0] for i in range(64)]  # headings cancel: infinite circular variance
    f.set_particles(states, np.ones(64))
    with pytest.raises(capi.MclError) as e:
        f.resample(0.5, step=1)
    assert e.value.status == capi.MCL_ERR_BAD_COVARIANCE
    assert np.array_equal(f.particles()[0], states)
    f.close()


def _track(grid, m, truth, start, odometry_noise, blind, cycles=50):
    origin = (grid.origin[2], grid.origin[3])
    gpu = Amcl(m, MOTION, NODE, AmclParams(min_particles=500, max_particles=2000), seed=0xBE1A6A)
    gpu.initialize(start, np.diag([0.09, 0.09, 0.02]))
    angles = synth.lidar_angles(360, 360.0)
    rng = np.random.Generator(np.random.PCG64(17))
    pose, odom = tuple(truth), (0.0, 0.0, 0.0)
    est = None
    for c in range(cycles):
        fwd, turn = 0.02, 0.12  # a circle of 0.17 m radius around the start, inside its clearance
        pose = synth.odometry_step(pose, fwd, turn)
        # what the wheels report: the true step with 10 % noise on the translation and 0.02 rad on the rotation
        odom = synth.odometry_step(odom, fwd * (1.0 + odometry_noise * rng.normal()), turn + 0.2 * odometry_noise * rng.normal())
        ranges = synth.cast_scan(grid.cells, grid.resolution, origin, pose, angles, 3.5, 0.01, seed=c)
        pts = np.zeros((0, 2)) if blind else synth.scan_points(ranges, angles)
        gpu.force_update()
        e = gpu.update(se2_from_xytheta(*odom), pts)
        est = e if e is not None else est
    gpu.close()
    ex, ey, et = est[0][2], est[0][3], math.atan2(est[0][1], est[0][0])
    return math.hypot(ex - pose[0], ey - pose[1]), abs(math.remainder(et - pose[2], 2 * math.pi))


def test_tracking_on_the_turtlebot_world():
    """50 cycles on the config-1 world (KLD 500 .. 2000 particles, 360 beams of 3.5 m, the node's NDT parameters), started 0.35 m and
    0.1 rad away from the truth, with noisy odometry: the NDT weights pull the estimate onto the truth; the same run without a scan
    (every weight 1) stays off.  The scans are cast in the occupancy grid of the world, so the NDT map is the project's own fit of that
    grid (synth.make_ndt_map, 0.5 m cells): the reference's HDF5 map of the same world was built in a frame about 0.8 m apart along x
    from the .pgm's (its likelihood over such scans peaks there)."""
    grid = turtlebot_grid()
    origin = (grid.origin[2], grid.origin[3])
    keys, means, covs = synth.make_ndt_map(grid.cells, grid.resolution, 0.5, origin_xy=origin, seed=1)
    m = NDTMap2d(keys, means, covs, 0.5)
    truth = np.array(synth.find_free_pose(grid.cells, grid.resolution, origin, seed=4, clearance_cells=10))
    start = truth + np.array([0.25, -0.25, 0.1])
    d, a = _track(grid, m, truth, start, 0.1, blind=False)
    assert d < 0.3 and a < 0.2, (d, a)
    d_blind, _ = _track(grid, m, truth, start, 0.1, blind=True)
    assert d_blind > 0.3 and d_blind > d + 0.1, (d_blind, d)


def test_error_codes():
    m = turtlebot_ndt()
    lib = capi.load()
    f = new_ndt(m, 100)
    for call, status in [(lambda: f.initialize_from_map(), capi.MCL_ERR_UNSUPPORTED),
                         (lambda: f.likelihood_field_origin(), None),
                         (lambda: f.update_map(turtlebot_grid()), capi.MCL_ERR_UNSUPPORTED),
                         (lambda: f.update_map_async(turtlebot_grid()), capi.MCL_ERR_UNSUPPORTED)]:
        if status is None:
            with pytest.raises(RuntimeError):
                call()
        else:
            with pytest.raises(capi.MclError) as e:
                call()
            assert e.value.status == status
    assert not f.has_likelihood_field()
    f._shape = (1, 1)
    with pytest.raises(capi.MclError) as e:
        f.likelihood_field()
    assert e.value.status == capi.MCL_ERR_UNSUPPORTED
    assert lib.mcl_comm_attach(f._ctx, 0, 1, None) == capi.MCL_ERR_UNSUPPORTED
    # bad maps
    for bad in [NDTMap2d(np.array([[0, 0], [0, 0]], dtype=np.int32), np.zeros((2, 2)), np.tile(np.eye(2), (2, 1, 1)), 1.0),
                NDTMap2d(np.array([[0, 0]], dtype=np.int32), np.zeros((1, 2)), np.eye(2)[None], 0.0),
                NDTMap2d(np.array([[0, 0]], dtype=np.int32), np.array([[np.nan, 0.0]]), np.eye(2)[None], 1.0),
                NDTMap2d(np.array([[0, 0]], dtype=np.int32), np.zeros((1, 2)), np.array([[[1.0, 0.5], [0.2, 1.0]]]), 1.0)]:
        with pytest.raises(capi.MclError) as e:
            f.update_map(bad)
        assert e.value.status == capi.MCL_ERR_INVALID_ARGUMENT
    far = NDTMap2d(np.array([[0, 0], [20000, 20000]], dtype=np.int32), np.zeros((2, 2)), np.tile(np.eye(2), (2, 1, 1)), 1.0)
    with pytest.raises(capi.MclError) as e:
        f.update_map(far)
    assert e.value.status == capi.MCL_ERR_UNSUPPORTED
    f.close()
    # an NDT context without a map
    params = AmclParams(min_particles=10, max_particles=10)
    cfg = capi.Config()
    lib.mcl_default_config(cfg)
    cfg.sensor_kind = capi.MCL_SENSOR_NDT
    cfg.amcl.min_particles = cfg.amcl.max_particles = params.max_particles
    import ctypes as C
    ctx = capi._ctx()
    assert lib.mcl_create(C.byref(cfg), C.byref(ctx)) == capi.MCL_OK
    pts = ring_scan((0, 0), 60)
    assert lib.mcl_reweight(ctx, pts.ctypes.data_as(capi.c_double_p), len(pts)) == capi.MCL_ERR_NOT_READY
    lib.mcl_destroy(ctx)
    # an NDT map on a likelihood-field context
    g = Amcl(turtlebot_grid(), MOTION, LikelihoodFieldModelParam(), AmclParams(min_particles=10, max_particles=10))
    keys = np.ascontiguousarray(m.cells, dtype=np.int32)
    st = lib.mcl_set_ndt_map(g._ctx, keys.ctypes.data_as(C.POINTER(C.c_int32)), np.ascontiguousarray(m.means).ctypes.data_as(capi.c_double_p),
                             np.ascontiguousarray(m.covariances.reshape(-1, 4)).ctypes.data_as(capi.c_double_p), len(keys), 1.0, None)
    assert st == capi.MCL_ERR_INVALID_ARGUMENT
    g.close()


def test_update_map_replaces_the_map_between_updates():
    m = turtlebot_ndt()
    f = new_ndt(m, 1000)
    states = synth.normal_particles(1000, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), seed=3)
    pts = ring_scan((0.0, 0.0), 360, seed=1)
    f.set_particles(states, np.ones(1000))
    f.reweight(pts)
    a = f.particles()[1]
    shifted = NDTMap2d(m.cells + 1, m.means + 1.0, m.covariances, 1.0)
    f.update_map(shifted)
    f.set_particles(states, np.ones(1000))
    f.reweight(pts)
    b = f.particles()[1]
    means, covs = ref.to_cells(pts, 1.0)
    np.testing.assert_allclose(b, ref.weights_vectorized(ref_map(shifted), states, means, covs, 0.01, 1.0, 0.6), rtol=1e-12)
    assert not np.array_equal(a, b)
    f.close()


def test_cpp_ndt_demo_matches_the_python_facade(tmp_path):
    lib_dir = os.path.join(ROOT, "beluga_amd", "lib")
    exe = tmp_path / "ndt_demo"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ndt_demo.cpp"), "-L", lib_dir, "-lbeluga_mcl", f"-Wl,-rpath,{lib_dir}",
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    cpp = np.array([[float(v) for v in line.split()] for line in out.stdout.strip().splitlines()])
    keys, means, covs = [], [], []
    for k in range(-4, 4):
        c = k + 0.5
        for key, mean, cov in [((k, -4), (c, -3.9), (0.08, 0, 0, 0.002)), ((k, 3), (c, 3.9), (0.08, 0, 0, 0.002)),
                               ((-4, k), (-3.9, c), (0.002, 0, 0, 0.08)), ((3, k), (3.9, c), (0.002, 0, 0, 0.08))]:
            if key not in keys:
                keys.append(key)
                means.append(mean)
                covs.append(np.reshape(cov, (2, 2)))
    py = Amcl(NDTMap2d(np.array(keys, dtype=np.int32), np.array(means), np.array(covs), 1.0), MOTION, NODE,
              AmclParams(min_particles=2000, max_particles=2000), seed=7)
    py.initialize((0.0, 0.0, 0.0), np.diag([0.04, 0.04, 0.01]))
    a = np.arange(180) * 2.0 * math.pi / 180.0
    t = 3.9 / np.maximum(np.abs(np.cos(a)), np.abs(np.sin(a)))
    scan = np.stack([t * np.cos(a), t * np.sin(a)], 1)
    rows = []
    for _ in range(4):
        py.force_update()
        e = py.update(se2_from_xytheta(0, 0, 0), scan)
        rows.append([e[0][2], e[0][3], math.atan2(e[0][1], e[0][0])])
    np.testing.assert_allclose(cpp, np.array(rows), rtol=0, atol=1e-12)
    py.close()
