"""A fleet of landmark and bearing filters through mcl_landmark_batch_update (AmclBatch.update_detections): every member bit for bit its
twin's lone update, three launches per cycle for the members that share them, the counters, and every refusal as the member's own."""
import numpy as np
import pytest

from beluga_amd import capi, synth
from beluga_amd.amcl import (Amcl, AmclBatch, AmclParams, BearingModelParam, LandmarkMap, LandmarkMapBoundaries, LikelihoodFieldModelParam,
                             OccupancyGrid, se2_from_xytheta)

from test_gpu_landmark import L_SENSOR, MOTION, scene, world_detections

pytestmark = pytest.mark.gpu

B_LEVEL = BearingModelParam(0.1, (0.0, 0.0, 0.0, 1.0, 0.1, 0.0, 0.5))
TRUTH = (-0.5, 0.3, 0.2)
COV = np.diag([0.09, 0.09, 0.04])


def lmap(seed):
    pos, cat, box = scene(seed=seed)
    return pos, cat, LandmarkMap(LandmarkMapBoundaries(*box), (pos, cat))


def spec(map_seed, bearing, min_p, max_p, seed, on=True, **params):
    pos, cat, m = lmap(map_seed)
    return dict(grid=m, motion=MOTION, sensor=B_LEVEL if bearing else L_SENSOR,
                params=AmclParams(min_particles=min_p, max_particles=max_p, **params), seed=seed, landmark_small_cycle=on), (pos, cat, bearing)


#         map bearing min   max   seed  switch  detections
FLEET = [(1, False, 2000, 2000, 31, True, 6),
         (2, True, 500, 2000, 32, True, 16),
         (3, False, 1, 1, 33, True, 5),
         (1, True, 4096, 4096, 34, True, 9),
         (2, False, 700, 700, 35, True, 0),      # no detection: no block in the shared reweight
         (3, False, 1000, 1000, 36, False, 7),   # the switch off: its own cycle inside the call
         (1, True, 5000, 5000, 37, True, 4),     # 5000 particles: its own cycle inside the call
         (2, False, 1500, 1500, 38, True, 12)]   # returns the cluster-based estimate
FUSED = [0, 1, 2, 3, 4, 7]
CLUSTER = 7


def test_every_member_is_its_twins_lone_update(cycles=5):
    specs, scenes = zip(*[spec(m, b, lo, hi, s, on) for m, b, lo, hi, s, on, _ in FLEET])
    batch = AmclBatch([dict(s) for s in specs])
    twins = [Amcl(**s) for s in specs]
    for f in list(batch.members) + twins:
        f.initialize(TRUTH, COV)
    for pair in (batch.members, twins):
        pair[CLUSTER].set_estimate_kind(True)
    rng = np.random.Generator(np.random.PCG64(8))
    odom, pose = (0.0, 0.0, 0.0), TRUTH
    before = {name: batch.counter(name) for name in ("kernel_launches", "landmark_launches", "members_landmark_fused", "members_fused",
                                                      "members_alone", "cycles", "cluster_launches", "members_cluster_fused")}
    assert all(v == 0 for v in before.values())
    for c in range(cycles):
        odom = synth.odometry_step(odom, 0.3, 0.05)
        pose = synth.odometry_step(pose, 0.3, 0.05)
        ctrl = se2_from_xytheta(*odom)
        dets = []
        for (pos, cat, bearing), row in zip(scenes, FLEET):
            dets.append(world_detections(pos, cat, pose, row[6], rng, 0.02, bearing, B_LEVEL.sensor_pose_in_robot if bearing else None))
        for f in list(batch.members) + twins:
            f.force_update()
        got = batch.update_detections([ctrl] * len(FLEET), dets)
        assert batch.statuses == [capi.MCL_OK] * len(FLEET)
        for i, (twin, member) in enumerate(zip(twins, batch.members)):
            want = twin.update(ctrl, dets[i])
            assert want is not None and got[i] is not None, (c, i)
            # (bit for bit: a set of one particle has a covariance of NaNs, which compare equal as bytes only)
            assert got[i][0].tobytes() == want[0].tobytes() and got[i][1].tobytes() == want[1].tobytes(), (c, i)
            assert batch.last_infos[i] == twin.last_info, (c, i)
            (gs, gw), (ws, ww) = member.particles(), twin.particles()
            assert np.array_equal(gs, ws) and np.array_equal(gw, ww), (c, i)
            for name in ("small_tail_launches", "landmark_wave_launches"):
                assert member.counter(name) == twin.counter(name), (c, i, name)
        assert batch.counter("kernel_launches") == 3 * (c + 1)
        assert batch.counter("landmark_launches") == c + 1
        assert batch.counter("members_landmark_fused") == len(FUSED) * (c + 1) == batch.counter("members_fused")
        assert batch.counter("members_alone") == (len(FLEET) - len(FUSED)) * (c + 1)
        assert batch.counter("cycles") == c + 1
        assert batch.counter("members_cluster_fused") == c + 1 and batch.counter("cluster_launches") == 2 * (c + 1)
    for i, member in enumerate(batch.members):
        assert member.counter("small_tail_launches") == (cycles if i in FUSED else 0), i
    assert batch.members[4].counter("landmark_wave_launches") == 0  # (no detection: no launch, lone or shared)
    assert batch.counter("beam_launches") == 0 and batch.ndt_counts() == (0, 0)
    for f in twins:
        f.close()
    batch.close()


def small_grid():
    cells = np.zeros((32, 32), dtype=np.int8)
    cells[0, :] = cells[-1, :] = cells[:, 0] = cells[:, -1] = 100
    return OccupancyGrid(cells=cells, resolution=0.1)


def test_refusals_are_the_members_own():
    U, I = capi.MCL_ERR_UNSUPPORTED, capi.MCL_ERR_INVALID_ARGUMENT
    pos, cat, m = lmap(1)
    params = AmclParams(min_particles=300, max_particles=300)
    landmark = dict(grid=m, motion=MOTION, sensor=L_SENSOR, params=params, landmark_small_cycle=True)
    batch = AmclBatch([dict(landmark, seed=1), dict(grid=small_grid(), motion=MOTION, sensor=LikelihoodFieldModelParam(), params=params, seed=2),
                       dict(landmark, seed=3), dict(grid=m, motion=MOTION, sensor=B_LEVEL, params=params, seed=4, landmark_small_cycle=True)])
    batch.members[0].initialize(TRUTH, COV)
    batch.members[1].initialize((1.6, 1.6, 0.0), np.diag([0.04, 0.04, 0.01]))
    batch.members[2].initialize(TRUTH, COV)
    batch.members[3].initialize(TRUTH, COV)
    rng = np.random.Generator(np.random.PCG64(8))
    ctrl = [se2_from_xytheta(0.3, 0.0, 0.05)] * 4
    good = world_detections(pos, cat, TRUTH, 6, rng, 0.02, False)
    good_b = world_detections(pos, cat, TRUTH, 6, rng, 0.02, True, B_LEVEL.sensor_pose_in_robot)
    sets = lambda: [f.particles() for f in batch.members]
    same = lambda a, b: np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])

    # a likelihood-field member: MCL_ERR_UNSUPPORTED, untouched; the others proceed
    before = sets()
    out = batch.update_detections(ctrl, [good, good, good, good_b], check=False)
    after = sets()
    assert batch.statuses == [capi.MCL_OK, U, capi.MCL_OK, capi.MCL_OK] and batch.last_status == U
    assert out[0] is not None and out[1] is None and out[2] is not None and out[3] is not None
    assert same(before[1], after[1]) and not same(before[0], after[0]) and not same(before[2], after[2]) and not same(before[3], after[3])
    assert batch.counter("members_landmark_fused") == 3 and batch.counter("kernel_launches") == 3

    # 65 detections, a value that is not finite: the member's own MCL_ERR_INVALID_ARGUMENT, untouched
    ctrl = [se2_from_xytheta(0.6, 0.0, 0.1)] * 4
    many = (np.ones((65, 3)), np.zeros(65, dtype=np.uint32))
    nan = (good_b[0].copy(), good_b[1])
    nan[0][2, 1] = np.nan
    before = after
    out = batch.update_detections(ctrl, [many, good, good, nan], check=False)
    after = sets()
    assert batch.statuses == [I, U, capi.MCL_OK, I]
    assert same(before[0], after[0]) and same(before[1], after[1]) and same(before[3], after[3]) and not same(before[2], after[2])
    assert out[0] is None and out[2] is not None and out[3] is None
    # ... and the motion was not consumed: the same control with good detections updates them now
    out = batch.update_detections(ctrl, [good, good, good, good_b], check=False)
    assert batch.statuses == [capi.MCL_OK, U, capi.MCL_OK, capi.MCL_OK] and out[0] is not None and out[3] is not None and out[2] is None

    # decreasing offsets, a null table: refused with no member moved
    before = sets()
    cycles = batch.counter("cycles")
    ctrl = np.array([se2_from_xytheta(0.9, 0.0, 0.15)] * 4)
    xyz, dcat = np.concatenate([good[0]] * 3), np.concatenate([good[1]] * 3)
    batch.update_detection_offsets(ctrl, xyz, dcat, [0, 8, 4, 12, 18])
    assert batch.last_status == I
    lib = capi.load()
    assert lib.mcl_landmark_batch_update(batch._batch, ctrl.ctypes.data_as(capi.c_double_p), xyz.ctypes.data_as(capi.c_double_p),
                                         dcat.ctypes.data_as(capi.c_u32_p), None, None, None, None) == I
    assert lib.mcl_landmark_batch_update(None, None, None, None, None, None, None, None) == I
    assert all(same(a, b) for a, b in zip(before, sets())) and batch.counter("cycles") == cycles

    # mcl_batch_update keeps refusing landmark and bearing members
    scan = np.array([[1.0, 0.0], [0.0, 1.0]])
    batch.update(list(ctrl), [scan] * 4, check=False)
    assert batch.statuses == [U, capi.MCL_OK, U, U]
    batch.close()
