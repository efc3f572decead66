"""The small cycle of the landmark and bearing models (mcl_set_landmark_small_cycle) on the GPU: the wave-per-particle kernels against
the lane-per-particle kernels, bit for bit; ties; the cycle against the oracle's stages; injection from the map's box; the switch on and
off; refusals.  Tolerances are test_gpu_landmark.py's: weights relative 1e-12 against the restatement, estimates 1e-9, covariance rtol
1e-8, counts and the KLD cut exact, ancestors equal except at CDF-step ties (at most 3 per cycle, each explained)."""
import ctypes as C
import math

import numpy as np
import pytest

from beluga_amd import capi, synth
from beluga_amd.amcl import (Amcl, AmclParams, BeamModelParam, BearingModelParam, LandmarkMap, LandmarkMapBoundaries, LandmarkModelParam,
                             LikelihoodFieldModelParam, NDTMap2d, NDTModelParam2d, OccupancyGrid, se2_from_xytheta)
from oracle import binding as orc

import landmark_reference as ref
from test_gpu_landmark import B_SENSOR, HASH, L_SENSOR, MOTION, MOTION_T, _tie_flips, restated, scene, world_detections
from test_landmark_cpu import IDENTITY

pytestmark = pytest.mark.gpu

SIZES = {10: 1, 11: 2, 12: 63, 13: 64, 14: 65, 15: 130}  # category -> landmarks; category 99 has none
EMPTY = 99
BOX = ((-14.0, -14.0, 0.0), (14.0, 14.0, 2.0))
KS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 32, 33, 63, 64]


def wide_scene(seed=2):
    """325 landmarks scattered over 24 m x 24 m in categories of 1, 2, 63, 64, 65 and 130, interleaved in map order."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cat = rng.permutation(np.concatenate([np.full(c, k) for k, c in SIZES.items()])).astype(np.uint32)
    pos = np.column_stack([rng.uniform(-12.0, 12.0, (len(cat), 2)), rng.uniform(0.0, 2.0, len(cat))])
    return pos, cat


def wide_detections(k, bearing, seed, with_empty):
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    d = np.column_stack([rng.uniform(-8.0, 8.0, (k, 2)), rng.uniform(-0.5, 1.5, k)])
    if bearing:
        d = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.5, 2.0, k)[:, None]
    cats = list(SIZES) + ([EMPTY] if with_empty else [])
    # every category in turn, starting somewhere else for every k; shuffled, so that the bearing model's sort by category moves places
    cat = rng.permutation(np.array([cats[(k + j) % len(cats)] for j in range(k)], dtype=np.uint32)) if k else np.zeros(0, dtype=np.uint32)
    return d, cat.astype(np.uint32)


def new_filter(pos, cat, n, sensor, box=BOX, **kw):
    return Amcl(LandmarkMap(LandmarkMapBoundaries(*box), (pos, cat)), MOTION, sensor,
                AmclParams(min_particles=kw.pop("min_particles", n), max_particles=n, **kw), seed=kw.pop("seed", 11))


def both_forms(f, bearing, states, w0, det, cat):
    """The weights of the lane-per-particle kernel (switch off) and of the wave-per-particle kernel (switch on), and the wave launches of each."""
    out = []
    for on in (False, True):
        f.set_landmark_small_cycle(on)
        assert f.landmark_small_cycle() == on
        before = f.counter("landmark_wave_launches")
        f.set_particles(states, w0)
        (f.reweight_bearings if bearing else f.reweight_landmarks)((det, cat))
        out.append((f.particles()[1], f.counter("landmark_wave_launches") - before))
    return out


# ---- 1. the bits of the wave kernels --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bearing", [False, True], ids=["landmark", "bearing"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4096])
def test_wave_kernels_return_the_lane_kernels_bits(bearing, n):
    pos, cat = wide_scene()
    sensor = B_SENSOR if bearing else L_SENSOR
    f = new_filter(pos, cat, n, sensor)
    states = synth.normal_particles(n, (0.5, -0.5, 0.0), (6.0, 6.0, 3.0), seed=n)
    w0 = np.random.Generator(np.random.PCG64(n)).uniform(0.5, 2.0, n)
    for k in KS:
        det, dcat = wide_detections(k, bearing, k, with_empty=not bearing)
        (lane, lane_launches), (wave, wave_launches) = both_forms(f, bearing, states, w0, det, dcat)
        assert np.array_equal(lane, wave), (k, np.flatnonzero(lane != wave)[:5])
        assert lane_launches == 0 and wave_launches == (1 if k else 0), k
        if k == 0:
            assert np.array_equal(wave, w0)
        else:
            assert np.all(np.isfinite(wave)) and np.all(wave > 0.0) and not np.array_equal(wave, w0)
    f.close()


@pytest.mark.parametrize("k", [1, 3, 16, 64])
def test_bearing_detection_of_a_category_without_landmarks_zeroes_every_weight_in_both_forms(k):
    pos, cat = wide_scene()
    n = 37
    f = new_filter(pos, cat, n, B_SENSOR)
    states = synth.normal_particles(n, (0.5, -0.5, 0.0), (6.0, 6.0, 3.0), seed=k)
    det, dcat = wide_detections(k, True, k, with_empty=False)
    dcat[k // 2] = EMPTY
    (lane, _), (wave, launches) = both_forms(f, True, states, np.full(n, 1.5), det, dcat)
    f.close()
    assert launches == 1 and np.all(lane == 0.0) and np.all(wave == 0.0)
    assert not np.any(np.signbit(wave))


@pytest.mark.parametrize("bearing", [False, True], ids=["landmark", "bearing"])
def test_both_forms_match_the_restatement_at_1000_particles(bearing, n=1000, k=16):
    pos, cat = wide_scene()
    sensor = B_SENSOR if bearing else L_SENSOR
    f = new_filter(pos, cat, n, sensor)
    states = synth.normal_particles(n, (0.5, -0.5, 0.0), (6.0, 6.0, 3.0), seed=n + k)
    w0 = np.random.Generator(np.random.PCG64(n)).uniform(0.5, 2.0, n)
    det, dcat = wide_detections(k, bearing, k, with_empty=not bearing)
    (lane, _), (wave, launches) = both_forms(f, bearing, states, w0, det, dcat)
    f.close()
    want, gaps = restated(bearing, ref.LandmarkMap(pos, cat, BOX), states, det, dcat, sensor)
    assert gaps.size == 0 or gaps.min() > 1e-9, f"smallest best-to-second gap {gaps.min()}"
    assert np.all(want > 1e-200) and np.all(np.isfinite(want)) and launches == 1
    np.testing.assert_allclose(lane, w0 * want, rtol=1e-12)
    np.testing.assert_allclose(wave, w0 * want, rtol=1e-12)
    assert np.array_equal(lane, wave)


@pytest.mark.parametrize("bearing", [False, True], ids=["landmark", "bearing"])
def test_4097_particles_take_the_lane_kernel(bearing):
    pos, cat = wide_scene()
    n = 4097
    f = new_filter(pos, cat, n, B_SENSOR if bearing else L_SENSOR)
    states = synth.normal_particles(n, (0.5, -0.5, 0.0), (6.0, 6.0, 3.0), seed=1)
    det, dcat = wide_detections(9, bearing, 9, with_empty=False)
    (lane, a), (still_lane, b) = both_forms(f, bearing, states, np.ones(n), det, dcat)
    f.close()
    assert a == 0 and b == 0 and np.array_equal(lane, still_lane)


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------------------
def group_of(k):
    P = 1
    while P < k:
        P *= 2
    return 64 // P


def tied_map(first, second, at, far):
    """130 landmarks of category 7: `first` at index at[0], `second` at index at[1], every other one far away."""
    pos = np.array([far(i) for i in range(130)], dtype=np.float64)
    pos[at[0]], pos[at[1]] = first, second
    return pos, np.full(130, 7, dtype=np.uint32)


@pytest.mark.parametrize("k", [1, 2, 8, 33])
def test_tied_candidates_pick_the_first_in_map_order_in_the_wave_kernel(k):
    g = group_of(k)
    assert g == {1: 64, 2: 32, 8: 8, 33: 1}[k]
    pairs = sorted({p for p in [(0, 1), (0, g), (1, g), (g - 1, g), (5, 129), (64, 65)] if p[0] < p[1]})
    sensor = LandmarkModelParam(sigma_range=0.5, sigma_bearing=0.25, random_prob=1e-4)
    box = ((-300.0, -300.0, 0.0), (300.0, 300.0, 2.0))
    n = 5
    states = np.repeat(np.asarray(IDENTITY, dtype=np.float64).reshape(1, 4), n, axis=0)
    det, dcat = np.tile([1.0, 0.0, 0.0], (k, 1)), np.full(k, 7, dtype=np.uint32)
    for at in pairs:
        out = []
        for first, second in (((3.0, 0.0, 0.0), (1.0, 2.0, 0.0)), ((1.0, 2.0, 0.0), (3.0, 0.0, 0.0))):
            pos, cat = tied_map(first, second, at, lambda i: (100.0 + i, 100.0, 0.0))
            f = new_filter(pos, cat, n, sensor, box=box)
            (lane, _), (wave, launches) = both_forms(f, False, states, np.ones(n), det, dcat)
            f.close()
            assert launches == 1 and np.array_equal(lane, wave), (k, at)
            assert len(set(wave)) == 1
            out.append(wave[0])
        # (squared distance 4 for both; the first in map order is the match: (3, 0, 0) straight ahead, or (1, 2, 0) off the bearing)
        term = math.exp(-4.0 / 0.5) + 1e-4
        want = 1.0
        for _ in range(k):
            want *= term
        assert out[0] == pytest.approx(want, rel=1e-12) and out[0] != out[1], (k, at)
    # the bearing model's tie: equal dot products are equal apertures, so the pick does not show in the value
    bdet = np.tile([1.0, 0.0, 1.0], (k, 1))
    for at in pairs:
        pos, cat = tied_map((2.0, 0.0, 0.0), (0.0, 0.0, 2.0), at, lambda i: (-100.0 - i, 50.0, 0.0))
        f = new_filter(pos, cat, n, BearingModelParam(sigma_bearing=0.5), box=box)
        (lane, _), (wave, launches) = both_forms(f, True, states, np.ones(n), bdet, dcat)
        f.close()
        assert launches == 1 and np.array_equal(lane, wave) and np.all(np.isfinite(wave)) and np.all(wave > 0.0), (k, at)


# ---- 3. the small cycle against the oracle's stages ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bearing", [False, True], ids=["landmark", "bearing"])
@pytest.mark.parametrize("min_p,max_p", [(2000, 2000), (500, 2000)], ids=["fixed", "kld"])
def test_small_cycle_matches_the_oracle_stages(bearing, min_p, max_p, cycles=6, seed=21):
    pos, cat, box = scene()
    sensor = BearingModelParam(0.1, (0.0, 0.0, 0.0, 1.0, 0.1, 0.0, 0.5)) if bearing else L_SENSOR
    rmap = ref.LandmarkMap(pos, cat, box)
    params = AmclParams(min_particles=min_p, max_particles=max_p, alpha_slow=0.0, alpha_fast=0.0)
    gpu = Amcl(LandmarkMap(LandmarkMapBoundaries(*box), (pos, cat)), MOTION, sensor, params, seed=seed, landmark_small_cycle=True)
    assert gpu.landmark_small_cycle()
    truth = (-0.5, 0.3, 0.2)
    cov = np.diag([0.09, 0.09, 0.04])
    gpu.initialize(truth, cov)
    states, w = orc.init_normal(max_p, truth, cov, seed)
    g0, _ = gpu.particles()
    np.testing.assert_allclose(g0, states, rtol=1e-12, atol=1e-12)
    states = g0.copy()
    odom, pose, prev = (0.0, 0.0, 0.0), truth, None
    rng = np.random.Generator(np.random.PCG64(4))
    for c in range(cycles):
        odom = synth.odometry_step(odom, 0.3, 0.05)
        pose = synth.odometry_step(pose, 0.3, 0.05)
        ctrl = se2_from_xytheta(*odom)
        det, dcat = world_detections(pos, cat, pose, 6, rng, 0.02, bearing, sensor.sensor_pose_in_robot if bearing else None)
        gpu.force_update()
        tails, waves = gpu.counter("small_tail_launches"), gpu.counter("landmark_wave_launches")
        est = gpu.update(ctrl, (det, dcat))
        assert est is not None
        assert gpu.counter("small_tail_launches") == tails + 1 and gpu.counter("landmark_wave_launches") == waves + 1, f"cycle {c}"
        sampler = orc.diffdrive_sampler(ctrl, prev if prev is not None else ctrl, MOTION_T)
        prev = ctrl
        states = orc.propagate(states, sampler, seed, c + 1)
        w = orc.normalize(w * restated(bearing, rmap, states, det, dcat, sensor)[0])[0]
        want, anc = orc.resample(states, w, min_p, max_p, 0.05, 3.0, HASH, 0.0, seed, c + 1)
        got, gw = gpu.particles()
        assert len(got) == len(want), f"cycle {c}: particle counts differ"
        assert np.all(gw == 1.0)
        assert _tie_flips(got, want, w, seed, c + 1, range(len(got))) <= 3, f"cycle {c}"
        om, oc = orc.estimate(got, np.ones(len(got)))
        np.testing.assert_allclose(est[0], om, atol=1e-9)
        np.testing.assert_allclose(est[1], oc, rtol=1e-8, atol=1e-9)
        states, w = got, np.ones(len(got))
    gpu.close()


# ---- 4. injection ------------------------------------------------------------------------------------------------------------------------
def test_small_cycle_with_injection_draws_from_the_box():
    pos, cat, box = scene()
    rmap = ref.LandmarkMap(pos, cat, box)
    n, seed = 4096, 21
    a_slow, a_fast = 0.001, 0.1
    gpu = Amcl(LandmarkMap(LandmarkMapBoundaries(*box), (pos, cat)), MOTION, L_SENSOR,
               AmclParams(min_particles=n, max_particles=n, alpha_slow=a_slow, alpha_fast=a_fast), seed=seed, landmark_small_cycle=True)
    truth = (-0.5, 0.3, 0.2)
    gpu.initialize(truth, np.diag([0.09, 0.09, 0.04]))
    states, w = gpu.particles()
    slow, fast = 2.0 / n, 0.5 / n
    gpu.debug_set_recovery_filters(slow, fast)
    odom, pose, prev = (0.0, 0.0, 0.0), truth, None
    rng = np.random.Generator(np.random.PCG64(4))
    injected = 0
    for c in range(3):
        odom = synth.odometry_step(odom, 0.3, 0.05)
        pose = synth.odometry_step(pose, 0.3, 0.05)
        ctrl = se2_from_xytheta(*odom)
        det, dcat = world_detections(pos, cat, pose, 6, rng, 0.02, False)
        gpu.force_update()
        est = gpu.update(ctrl, (det, dcat))
        assert est is not None and gpu.counter("small_tail_launches") == c + 1
        sampler = orc.diffdrive_sampler(ctrl, prev if prev is not None else ctrl, MOTION_T)
        prev = ctrl
        states = orc.propagate(states, sampler, seed, c + 1)
        w = orc.normalize(w * restated(False, rmap, states, det, dcat, L_SENSOR)[0])[0]
        avg = w.sum() / len(w)  # ThrunRecoveryProbabilityEstimator on the normalised weights
        slow = avg if slow == 0.0 else slow + a_slow * (avg - slow)
        fast = avg if fast == 0.0 else fast + a_fast * (avg - fast)
        p = min(max(1.0 - fast / slow, 0.0), 1.0) if slow != 0.0 else 0.0
        assert gpu.last_info["random_state_probability"] == pytest.approx(p, abs=1e-12), f"cycle {c}"
        p = gpu.last_info["random_state_probability"]
        if p > 0.0:
            slow = fast = 0.0
        want, anc = orc.resample(states, w, n, n, 0.05, 3.0, HASH, p, seed, c + 1, free_xy=np.zeros((1, 2)))
        got, gw = gpu.particles()
        assert len(got) == len(want) == n and np.all(gw == 1.0)
        inj = anc == -1
        injected += int(inj.sum())
        assert _tie_flips(got, want, w, seed, c + 1, np.flatnonzero(~inj)) <= 3, f"cycle {c}"
        if inj.any():
            slots = np.flatnonzero(inj)
            np.testing.assert_allclose(got[slots], ref.box_states(rmap, seed, c + 1, slots), rtol=1e-12, atol=1e-12)
        states, w = got, np.ones(n)
    assert injected > 100
    gpu.close()


# ---- 5. the switch on and off --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bearing", [False, True], ids=["landmark", "bearing"])
def test_switch_on_and_off_agree(bearing):
    """A cycle that does not resample (resample_interval 1000): the set behind it is the propagated one with the normalised weights."""
    pos, cat, box = scene()
    sensor = BearingModelParam(0.1, (0.0, 0.0, 0.0, 1.0, 0.1, 0.0, 0.5)) if bearing else L_SENSOR
    n = 2000
    rng = np.random.Generator(np.random.PCG64(4))
    det, dcat = world_detections(pos, cat, (-0.2, 0.3, 0.25), 6, rng, 0.02, bearing, sensor.sensor_pose_in_robot if bearing else None)
    out = []
    for on in (False, True, True):
        f = Amcl(LandmarkMap(LandmarkMapBoundaries(*box), (pos, cat)), MOTION, sensor,
                 AmclParams(min_particles=n, max_particles=n, resample_interval=1000), seed=5, landmark_small_cycle=on)
        f.initialize((-0.5, 0.3, 0.2), np.diag([0.09, 0.09, 0.04]))
        est = None
        for step in (1, 2):
            f.force_update()
            est = f.update(se2_from_xytheta(0.3 * step, 0.0, 0.05 * step), (det, dcat))
        assert est is not None and f.counter("small_tail_launches") == (2 if on else 0)
        assert not f.last_info["resampled"]
        states, w = f.particles()
        out.append((states, w, est))
        f.close()
    (s_off, w_off, e_off), (s_on, w_on, e_on), (s_again, w_again, e_again) = out
    assert np.array_equal(s_off, s_on)
    np.testing.assert_allclose(w_on, w_off, rtol=1e-12)
    assert w_on.sum() == pytest.approx(1.0, rel=1e-12) and w_on.max() > 0.0
    np.testing.assert_allclose(e_on[0], e_off[0], atol=1e-9)
    np.testing.assert_allclose(e_on[1], e_off[1], rtol=1e-8, atol=1e-9)
    assert np.array_equal(s_on, s_again) and np.array_equal(w_on, w_again)
    assert np.array_equal(e_on[0], e_again[0]) and np.array_equal(e_on[1], e_again[1])


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = capi.load()
    U, I = capi.MCL_ERR_UNSUPPORTED, capi.MCL_ERR_INVALID_ARGUMENT
    cells = np.zeros((32, 32), dtype=np.int8)
    cells[0, :] = cells[-1, :] = cells[:, 0] = cells[:, -1] = 100
    grid = OccupancyGrid(cells=cells, resolution=0.1)
    keys = np.array([[x, y] for x in range(4) for y in range(4)], dtype=np.int32)
    ndt = NDTMap2d(keys, keys + 0.5, np.tile(np.eye(2) * 0.05, (16, 1, 1)), 1.0)
    params = AmclParams(min_particles=64, max_particles=64)
    on = C.c_int32(7)
    for m, sensor in ((grid, LikelihoodFieldModelParam()), (grid, BeamModelParam()), (ndt, NDTModelParam2d())):
        f = Amcl(m, MOTION, sensor, params, seed=3)
        assert lib.mcl_set_landmark_small_cycle(f._ctx, 1) == U and lib.mcl_set_landmark_small_cycle(f._ctx, 0) == U
        assert lib.mcl_get_landmark_small_cycle(f._ctx, C.byref(on)) == U and on.value == 7
        with pytest.raises(capi.MclError) as e:
            f.set_landmark_small_cycle(True)
        assert e.value.status == U
        f.close()
        with pytest.raises(ValueError):
            Amcl(m, MOTION, sensor, params, seed=3, landmark_small_cycle=True)
    assert lib.mcl_set_landmark_small_cycle(None, 1) == I and lib.mcl_get_landmark_small_cycle(None, C.byref(on)) == I
    pos, cat, box = scene()
    for sensor in (L_SENSOR, B_SENSOR):
        f = Amcl(LandmarkMap(LandmarkMapBoundaries(*box), (pos, cat)), MOTION, sensor, params, seed=3)
        assert not f.landmark_small_cycle()  # (off by default)
        for value in (2, -1, 256):
            assert lib.mcl_set_landmark_small_cycle(f._ctx, value) == I
            assert not f.landmark_small_cycle()
        assert lib.mcl_get_landmark_small_cycle(f._ctx, None) == I
        f.set_landmark_small_cycle(True)
        assert lib.mcl_set_landmark_small_cycle(f._ctx, 2) == I and f.landmark_small_cycle()
        f.set_landmark_small_cycle(False)
        assert not f.landmark_small_cycle()
        f.close()


@pytest.mark.parametrize("bearing", [False, True], ids=["landmark", "bearing"])
def test_4097_particles_take_the_general_path(bearing):
    pos, cat, box = scene()
    sensor = BearingModelParam(0.1, (0.0, 0.0, 0.0, 1.0, 0.1, 0.0, 0.5)) if bearing else L_SENSOR
    n = 4097
    f = Amcl(LandmarkMap(LandmarkMapBoundaries(*box), (pos, cat)), MOTION, sensor, AmclParams(min_particles=n, max_particles=n), seed=5,
             landmark_small_cycle=True)
    f.initialize((-0.5, 0.3, 0.2), np.diag([0.09, 0.09, 0.04]))
    rng = np.random.Generator(np.random.PCG64(4))
    det, dcat = world_detections(pos, cat, (-0.2, 0.3, 0.25), 6, rng, 0.02, bearing, sensor.sensor_pose_in_robot if bearing else None)
    f.force_update()
    assert f.update(se2_from_xytheta(0.3, 0.0, 0.05), (det, dcat)) is not None
    assert f.counter("small_tail_launches") == 0 and f.counter("landmark_wave_launches") == 0 and f.last_info["resampled"]
    f.close()
