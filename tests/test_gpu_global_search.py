"""mcl_global_search*: every free cell and heading scored with the sensor model on the device, the best kept.

The reference is tests/search_reference.py over the scores mcl_likelihoods gives for the same poses: the search promises those bits.
  1. enumeration: cells, ids and positions equal the reference's, bit for bit; the rotations within 2^-52 of numpy's cos / sin and
     identical among the cells of a heading;
  2. scores: the pool of a search that keeps every candidate has mcl_likelihoods' bits, in pool order (LF, LF-prob, beam; 0 .. 180
     points, one of them NaN); a subset against the CPU oracle at the relative 1e-12 tests/test_gpu_likelihoods.py derives;
  3. selection: ~1e5 candidates, pools 1 .. 4096, three chunk sizes - one pool, the reference's, and the chunk plan's count;
  4. ties: every score equal -> the lowest ids; a hall whose pool-th score is shared across the cut and across a chunk boundary;
  5. the suppression end to end; 6. the kidnapped robot; 7. the filter untouched; 8. refusals.
"""
import ctypes as C
import math

import numpy as np
import pytest

import search_reference as ref
from beluga_amd import capi, synth
from beluga_amd.amcl import (Amcl, AmclBatch, AmclParams, BeamModelParam, BearingModelParam, DifferentialDriveModelParam, LandmarkMap,
                             LandmarkMapBoundaries, LandmarkModelParam, LandmarkPositionDetection, LikelihoodFieldModelParam,
                             LikelihoodFieldProbModelParam, NDTModelParam2d, OccupancyGrid, SharedMap, load_ndt_map_npz, se2_from_xytheta)
from oracle import binding as orc

pytestmark = pytest.mark.gpu

RTOL = 1e-12  # tests/test_gpu_likelihoods.py: (B + 4) 2^-53 < 1.3e-13 at B = 1080
MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
LF = LikelihoodFieldModelParam(max_obstacle_distance=2.0, max_laser_distance=100.0, z_hit=0.5, z_random=0.5, sigma_hit=0.2, model_unknown_space=True)
LF_PROB = LikelihoodFieldProbModelParam(max_obstacle_distance=2.0, max_laser_distance=100.0, z_hit=0.5, z_random=0.5, sigma_hit=0.2,
                                        model_unknown_space=True)
BEAM = BeamModelParam(0.5, 0.05, 0.05, 0.5, 0.2, 0.1, 60.0)
BEAM_T = (0.5, 0.05, 0.05, 0.5, 0.2, 0.1, 60.0)
SMALL = AmclParams(max_particles=64)
COV = np.diag([0.25, 0.25, 0.04])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rooms(width, height, seed, n_rooms, origin=None, resolution=0.05):
    cells = synth.make_rooms_map(width, height, seed=seed, n_rooms=n_rooms)
    return OccupancyGrid(cells=cells, resolution=resolution, origin=se2_from_xytheta(*(origin or (-width * resolution / 2, -height * resolution / 2, 0.0))))


def world_xytheta(grid, x_cell, y_cell, theta):
    gx, gy = ref.cell_positions([y_cell * grid.cells.shape[1] + x_cell], grid.cells.shape[1], grid.resolution, grid.origin)
    return (float(gx[0]), float(gy[0]), theta)


def local_scan(grid, pose, beams, max_range=12.0, seed=1):
    """A scan cast from `pose` (world x, y, theta) on a grid whose origin may be rotated: cast in the grid's own frame."""
    if beams == 0:
        return np.zeros((0, 2))
    c, s, ox, oy = (float(v) for v in grid.origin)
    dx, dy = pose[0] - ox, pose[1] - oy
    local = (c * dx + s * dy, -s * dx + c * dy, pose[2] - math.atan2(s, c))
    angles = synth.lidar_angles(beams, 270.0)
    ranges = synth.cast_scan(grid.cells, grid.resolution, (0.0, 0.0), local, angles, max_range, 0.0, seed)
    return synth.scan_points(ranges, angles)


def free_pose(grid, seed, clearance=4):
    c, s, ox, oy = (float(v) for v in grid.origin)
    lx, ly, t = synth.find_free_pose(grid.cells, grid.resolution, (0.0, 0.0), seed=seed, clearance_cells=clearance)
    return (c * lx - s * ly + ox, s * lx + c * ly + oy, t + math.atan2(s, c))


def all_candidates(f, grid, stride, headings):
    ids, poses, total = f.search_candidates(stride, headings)
    assert total == len(ids)
    return ids, poses


def pool_arrays(hits):
    return (np.array([h.id for h in hits], dtype=np.uint64), np.array([h.score for h in hits], dtype=np.float64),
            np.array([h.pose for h in hits], dtype=np.float64).reshape(-1, 4))


# ---- 1. enumeration ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", [(-3.7, 2.9, 0.6), (1.0e6 - 4.0, -2.0e6 - 4.0, 0.3)], ids=["offset_rotated", "far"])
def test_enumeration_equals_the_reference(origin):
    grid = rooms(24, 20, 3, 2, origin=origin)
    f = Amcl(grid, MOTION, LF, SMALL, seed=1, options={"search_chunk": 64})
    W = grid.cells.shape[1]
    for stride, headings in ((1, 7), (2, 72), (3, 1), (25, 5)):
        ids, poses, total = f.search_candidates(stride, headings)
        cells = ref.candidate_cells(grid.cells, grid.value_traits[0], stride)
        if stride == 25:  # cell (0, 0) is a wall: no cell left
            assert len(cells) == 0
        assert total == len(cells) * headings
        assert np.array_equal(ids, ref.candidate_ids(cells, headings))
        x, y = ref.cell_positions(cells, W, grid.resolution, grid.origin)
        assert np.array_equal(bits(poses[:, 2]), bits(np.repeat(x, headings))) and np.array_equal(bits(poses[:, 3]), bits(np.repeat(y, headings)))
        theta = np.tile(ref.heading_angles(headings), len(cells))
        assert np.all(np.abs(poses[:, 0] - np.cos(theta)) <= 2.0 ** -52) and np.all(np.abs(poses[:, 1] - np.sin(theta)) <= 2.0 ** -52)
        if len(cells):
            rot = bits(poses[:, :2]).reshape(len(cells), headings, 2)
            assert np.array_equal(rot, np.broadcast_to(rot[:1], rot.shape))
            # a window of the list, across chunk boundaries
            first, count = 5, min(3 * headings + 1, total - 5)
            some_ids, some_poses, again = f.search_candidates(stride, headings, first=first, count=count)
            assert again == total and np.array_equal(some_ids, ids[first:first + count])
            assert np.array_equal(bits(some_poses), bits(poses[first:first + count]))
    f.close()


# ---- 2. scores ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_world():
    grid = rooms(24, 20, 3, 2, origin=(-3.7, 2.9, 0.6))
    return grid, free_pose(grid, 2, clearance=2)


@pytest.mark.parametrize("sensor", [LF, LF_PROB, BEAM], ids=["lf", "lf_prob", "beam"])
def test_pool_of_everything_has_mcl_likelihoods_bits(small_world, sensor):
    grid, truth = small_world
    f = Amcl(grid, MOTION, sensor, SMALL, seed=1)
    stride, headings = 2, 16
    ids, poses = all_candidates(f, grid, stride, headings)
    assert 0 < len(ids) <= 4096
    for beams in (0, 1, 63, 64, 65, 180):
        pts = local_scan(grid, truth, beams, max_range=6.0)
        if beams == 65:
            pts[7, 0] = np.nan  # a point without a cell for any pose
        want = f.likelihoods(poses, pts)
        order = ref.pool_order(ids, want, 4096)
        for chunk in (64, 1 << 20):
            f.set_option("search_chunk", chunk)
            got_ids, got_scores, got_poses = pool_arrays(f.global_search_pool(pts, stride, headings, 4096))
            assert f.last_search_info["pool_filled"] == len(ids) == f.last_search_info["candidates"]
            assert np.array_equal(got_ids, ids[order]), (beams, chunk)
            assert np.array_equal(bits(got_scores), bits(want[order])), (beams, chunk)
            assert np.array_equal(bits(got_poses), bits(poses[order])), (beams, chunk)
        # a subset against the CPU oracle
        if beams in (1, 180):
            sub = poses[:: max(1, len(poses) // 97)]
            if sensor is BEAM:
                oracle = orc.beam_weights(grid.cells, grid.resolution, grid.origin, BEAM_T, sub, pts)
            else:
                oracle = orc.lf_weights(f.likelihood_field(), grid.resolution, grid.origin, LF.max_laser_distance, sub, pts)
                if sensor is LF_PROB:
                    continue  # (the oracle's function is the plain model's)
            np.testing.assert_allclose(f.likelihoods(sub, pts), oracle, rtol=RTOL, atol=0)
    f.close()


# ---- 3. selection, 4. ties ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide_world():
    """96 x 80 rooms, stride 1, 16 headings: about 1e5 candidates, scored once by mcl_likelihoods."""
    grid = rooms(96, 80, 7, 4)
    truth = free_pose(grid, 3, clearance=3)
    pts = local_scan(grid, truth, 64, max_range=6.0)
    f = Amcl(grid, MOTION, LF, SMALL, seed=1)
    ids, poses = all_candidates(f, grid, 1, 16)
    scores = f.likelihoods(poses, pts)
    f.close()
    return grid, pts, ids, poses, scores


def test_selection_is_the_reference_for_every_pool_and_chunk(wide_world):
    grid, pts, ids, poses, scores = wide_world
    assert 50_000 < len(ids) < 130_000
    free_cells = int(np.count_nonzero(grid.cells == grid.value_traits[0]))
    f = Amcl(grid, MOTION, LF, SMALL, seed=1)
    for pool in (1, 63, 64, 65, 1000, 4096):
        order = ref.pool_order(ids, scores, pool)
        for chunk in (64, 4096, 1 << 20):
            f.set_option("search_chunk", chunk)
            got_ids, got_scores, _ = pool_arrays(f.global_search_pool(pts, 1, 16, pool))
            assert np.array_equal(got_ids, ids[order]), (pool, chunk)
            assert np.array_equal(bits(got_scores), bits(scores[order])), (pool, chunk)
            info = f.last_search_info
            assert info["chunks"] == ref.chunk_plan(free_cells, 16, chunk)[1] and info["candidates"] == len(ids) and info["pool_filled"] == pool
            assert info["launches"] >= 4
    f.close()


def test_equal_scores_keep_the_lowest_ids(wide_world):
    grid, _, ids, _, _ = wide_world
    f = Amcl(grid, MOTION, LF, SMALL, seed=1)
    for chunk in (64, 4096, 1 << 20):
        f.set_option("search_chunk", chunk)
        for pool in (1, 65, 4096):
            got_ids, got_scores, _ = pool_arrays(f.global_search_pool(np.zeros((0, 2)), 1, 16, pool))
            assert np.array_equal(got_ids, ids[:pool]) and np.all(got_scores == got_scores[0])
    f.close()


def hall_world():
    """An open hall: walls on the border alone.  A short scan scores the same, bit for bit, at every pose whose end-points all lie
    further than max_obstacle_distance from the walls, and along a wall every cell at the same distance from it ties as well."""
    cells = np.zeros((50, 60), dtype=np.int8)
    cells[0, :] = cells[-1, :] = cells[:, 0] = cells[:, -1] = 100
    grid = OccupancyGrid(cells=cells, resolution=0.1, origin=se2_from_xytheta(-3.0, -2.5, 0.0))
    pts = np.array([[0.35, 0.0], [0.0, 0.35], [-0.35, 0.0]])
    return grid, pts


HALL_LF = LikelihoodFieldModelParam(max_obstacle_distance=0.5, max_laser_distance=100.0, z_hit=0.5, z_random=0.5, sigma_hit=0.2, model_unknown_space=True)


def test_ties_across_the_cut_and_across_chunks():
    """Headings 4: the axis-aligned headings make whole rows of cells along a wall tie exactly.  Checked on the CPU with the oracle's
    scores (orc.lf_weights over these candidates) before the pool sizes were fixed: both assertions on the reference scores held."""
    grid, pts = hall_world()
    headings, W = 4, grid.cells.shape[1]
    f = Amcl(grid, MOTION, HALL_LF, SMALL, seed=1)
    ids, poses = all_candidates(f, grid, 1, headings)
    scores = f.likelihoods(poses, pts)
    free = ref.candidate_cells(grid.cells, 0, 1)
    per_chunk = ref.chunk_plan(len(free), headings, 64)[0]
    rank_of_cell = {int(c): k for k, c in enumerate(free)}
    for pool in (100, 1000, 4096):
        order = ref.pool_order(ids, scores, len(ids))
        cut = scores[order[pool - 1]]
        tied = order[scores[order] == cut]
        position = {int(i): k for k, i in enumerate(order)}
        assert any(position[int(i)] < pool for i in tied) and any(position[int(i)] >= pool for i in tied), pool  # both sides of the cut
        chunks = {rank_of_cell[int(ids[i]) // headings] // per_chunk for i in tied}
        assert len(chunks) > 1, pool  # the run of equal scores crosses a chunk boundary
        for chunk in (64, 4096, 1 << 20):
            f.set_option("search_chunk", chunk)
            got_ids, got_scores, _ = pool_arrays(f.global_search_pool(pts, 1, headings, pool))
            assert np.array_equal(got_ids, ids[order[:pool]]), (pool, chunk)
            assert np.array_equal(bits(got_scores), bits(scores[order[:pool]])), (pool, chunk)
    f.close()


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------------
def test_global_search_is_the_reference_suppression_of_the_pool(wide_world):
    grid, pts, ids, poses, scores = wide_world
    W = grid.cells.shape[1]
    f = Amcl(grid, MOTION, LF, SMALL, seed=1)
    pool_hits = f.global_search_pool(pts, 1, 16, 1024)
    cells, heads = [h.cell for h in pool_hits], [h.heading for h in pool_hits]
    assert all(h.id == h.cell * 16 + h.heading for h in pool_hits)
    for sep_xy, sep_theta, most in ((0.5, math.radians(30), 16), (0.0, 0.0, 16), (0.2, math.radians(45), 1), (0.3, math.pi, 1024)):
        sep_cells, sep_heads = int(round(sep_xy / grid.resolution)), int(round(sep_theta / (2 * math.pi / 16)))
        kept = ref.suppress(cells, heads, W, 16, sep_cells, sep_heads, most)
        hits = f.global_search(pts, 1, 16, 1024, most, sep_xy, sep_theta)
        assert [h.id for h in hits] == [pool_hits[k].id for k in kept]
        assert all(np.array_equal(bits(h.pose), bits(pool_hits[k].pose)) and h.score == pool_hits[k].score for h, k in zip(hits, kept))
        if (sep_xy, most) == (0.5, 16):
            assert kept != list(range(len(kept)))  # the pool has near-duplicates of its peaks: something was dropped
    f.close()


# ---- 6. the scenario -----------------------------------------------------------------------------------------------------------------------
def test_kidnapped_robot_is_found_and_tracked():
    """200 x 200 rooms, a noise-free 180-beam scan from a pose at a candidate (even cell, a multiple of 5 degrees), stride 2, 72 headings.
    Map seed and pose were checked on the CPU first: orc.lf_weights over all candidates of this map and scan puts the truth's own
    candidate first (the map is not symmetric)."""
    grid = rooms(200, 200, 5, 8)
    H, W = grid.cells.shape
    lx, ly, _ = synth.find_free_pose(grid.cells, grid.resolution, (0.0, 0.0), seed=3, clearance_cells=6)
    xc, yc = int(lx / grid.resolution) // 2 * 2, int(ly / grid.resolution) // 2 * 2
    assert grid.cells[yc, xc] == 0
    heading = 47
    truth = world_xytheta(grid, xc, yc, -math.pi + heading * (2 * math.pi / 72))
    angles = synth.lidar_angles(180, 270.0)
    scan_of = lambda pose, seed: synth.scan_points(synth.cast_scan(grid.cells, grid.resolution, (grid.origin[2], grid.origin[3]), pose, angles, 8.0, 0.0, seed), angles)
    params = AmclParams(min_particles=500, max_particles=2000, update_min_d=0.0, update_min_a=0.0, resample_interval=1)
    f = Amcl(grid, MOTION, LF, params, seed=11)
    hits = f.relocalize(scan_of(truth, 0), np.diag([0.01, 0.01, 0.005]))
    best = hits[0]
    assert abs(best.cell % W - xc) <= 2 and abs(best.cell // W - yc) <= 2
    dh = abs(best.heading - heading)
    assert min(dh, 72 - dh) <= 1
    pose, odom = truth, (0.0, 0.0, 0.0)
    for c in range(3):
        pose, odom = synth.odometry_step(pose, 0.1, 0.02), synth.odometry_step(odom, 0.1, 0.02)
        est = f.update(se2_from_xytheta(*odom), scan_of(pose, c))
        assert est is not None
        x, y = est[0][2], est[0][3]
        theta = math.atan2(est[0][1], est[0][0])
        assert math.hypot(x - pose[0], y - pose[1]) < 0.9
        assert abs(math.remainder(theta - pose[2], 2 * math.pi)) < math.radians(30)
    f.close()


# ---- 7. the filter is untouched --------------------------------------------------------------------------------------------------------------
CYCLE_COUNTERS = ("lf_fast_launches", "lf_patch_launches", "lf_beams_launches", "lf_far_launches", "small_tail_launches", "field_pose_rebuilds",
                  "estimate_repivots", "noise_ahead_used", "order_ahead_used", "order_ahead_missed")


def snapshot(f):
    s, w = f.particles()
    counters = {}
    for name in CYCLE_COUNTERS:
        try:
            counters[name] = f.counter(name)
        except capi.MclError:
            pass
    return bits(s).tobytes(), bits(w).tobytes(), f.last_info, counters


def run_twins(asked, twin, grid, truth, cycles=3):
    scan_of = lambda pose, seed: local_scan(grid, pose, 65, max_range=6.0, seed=seed)
    assert asked.global_search(scan_of(truth, 0), 2, 8, 256, 4)
    pose, odom = truth, (0.0, 0.0, 0.0)
    for c in range(cycles):
        pose, odom = synth.odometry_step(pose, 0.1, 0.02), synth.odometry_step(odom, 0.1, 0.02)
        pts = scan_of(pose, c)
        a, b = asked.update(se2_from_xytheta(*odom), pts), twin.update(se2_from_xytheta(*odom), pts)
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])), c
        assert snapshot(asked) == snapshot(twin), c
        assert asked.global_search(pts, 2, 8, 256, 4)
        assert snapshot(asked) == snapshot(twin), c


@pytest.fixture(scope="module")
def twin_world():
    grid = rooms(96, 80, 7, 4)
    return grid, free_pose(grid, 3, clearance=3)


TWIN_PARAMS = AmclParams(min_particles=500, max_particles=2000, update_min_d=0.0, update_min_a=0.0, resample_interval=1)


def test_untouched_own_map_and_shared_map(twin_world):
    grid, truth = twin_world
    pair = [Amcl(grid, MOTION, LF, TWIN_PARAMS, seed=42) for _ in range(2)]
    for f in pair:
        f.initialize(truth, COV)
    run_twins(pair[0], pair[1], grid, truth)
    shared = SharedMap(grid, LF)
    on_shared = [Amcl(grid, MOTION, LF, TWIN_PARAMS, seed=42) for _ in range(2)]
    for f in on_shared:
        f.use_map(shared)
        f.initialize(truth, COV)
    run_twins(on_shared[0], on_shared[1], grid, truth)
    pts = local_scan(grid, truth, 65, max_range=6.0)
    assert [h.id for h in on_shared[0].global_search(pts, 2, 8, 256, 4)] == [h.id for h in pair[0].global_search(pts, 2, 8, 256, 4)]
    for f in pair + on_shared:
        f.close()
    shared.close()


def test_untouched_member_of_a_batch(twin_world):
    grid, truth = twin_world
    params = AmclParams(min_particles=500, max_particles=1000, update_min_d=0.0, update_min_a=0.0, resample_interval=1)
    specs = [dict(grid=grid, motion=MOTION, sensor=LF, params=params, seed=20 + k) for k in range(3)]
    fleets = [AmclBatch(specs) for _ in range(2)]
    for fleet in fleets:
        for m in fleet.members:
            m.initialize(truth, COV)
    asked = fleets[0].members[1]
    lone = Amcl(grid, MOTION, LF, SMALL, seed=1)
    pose, odom = truth, (0.0, 0.0, 0.0)
    for c in range(3):
        pts = local_scan(grid, pose, 65, max_range=6.0, seed=c)
        assert [h.id for h in asked.global_search(pts, 2, 8, 256, 4)] == [h.id for h in lone.global_search(pts, 2, 8, 256, 4)]
        pose, odom = synth.odometry_step(pose, 0.1, 0.02), synth.odometry_step(odom, 0.1, 0.02)
        pts = local_scan(grid, pose, 65, max_range=6.0, seed=c)
        results = [fleet.update([se2_from_xytheta(*odom)] * 3, [pts] * 3) for fleet in fleets]
        for a, b in zip(*results):
            assert (a is None) == (b is None)
            if a is not None:
                assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])), c
        for a, b in zip(fleets[0].members, fleets[1].members):
            assert snapshot(a) == snapshot(b), c
        assert fleets[0].last_infos == fleets[1].last_infos
    lone.close()
    for fleet in fleets:
        fleet.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------
def raw_search(f, fn, pts, params, capacity, hits=True, count=True, null_points=False, null_ctx=False):
    lib = capi.load()
    sentinel = 0x5A
    buf = (capi.SearchHit * 4100)()
    C.memset(buf, sentinel, C.sizeof(buf))
    n = C.c_uint64(0xDEADBEEF)
    info = capi.SearchInfo()
    C.memset(C.byref(info), sentinel, C.sizeof(info))
    p = None if pts is None else np.ascontiguousarray(pts, dtype=np.float64)
    status = getattr(lib, fn)(None if null_ctx else f._ctx, None if p is None or null_points else p.ctypes.data_as(capi.c_double_p), 0 if p is None else len(p),
                              C.byref(params) if params is not None else None, buf if hits else None, capacity, C.byref(n) if count else None,
                              C.byref(info))
    untouched = bytes(buf) == bytes([sentinel]) * C.sizeof(buf) and n.value == 0xDEADBEEF and bytes(info) == bytes([sentinel]) * C.sizeof(info)
    return status, untouched


def test_refusals_leave_the_outputs_as_they_were(small_world):
    grid, truth = small_world
    pts = local_scan(grid, truth, 16, max_range=6.0)
    P = capi.SearchParams
    f = Amcl(grid, MOTION, LF, SMALL, seed=1)
    bad = [P(0, 8, 16, 4, 0, 0), P(1, 0, 16, 4, 0, 0), P(1, 4097, 16, 4, 0, 0), P(1, 8, 0, 1, 0, 0), P(1, 8, 4097, 4, 0, 0), P(1, 8, 16, 0, 0, 0),
           P(1, 8, 16, 17, 0, 0)]
    for fn in ("mcl_global_search", "mcl_global_search_pool"):
        for params in bad:
            assert raw_search(f, fn, pts, params, 4100) == (capi.MCL_ERR_INVALID_ARGUMENT, True), (fn, list(bytes(params)))
        good = P(1, 8, 16, 4, 0, 0)
        assert raw_search(f, fn, pts, good, 4100, hits=False) == (capi.MCL_ERR_INVALID_ARGUMENT, True)
        assert raw_search(f, fn, pts, good, 4100, count=False) == (capi.MCL_ERR_INVALID_ARGUMENT, True)
        assert raw_search(f, fn, pts, good, 3 if fn == "mcl_global_search" else 15) == (capi.MCL_ERR_INVALID_ARGUMENT, True)
        assert raw_search(f, fn, pts, good, 4 if fn == "mcl_global_search" else 16)[0] == capi.MCL_OK
        assert raw_search(f, fn, pts, None, 4100)[0] == capi.MCL_OK  # NULL: the defaults
        assert raw_search(f, fn, pts, good, 4100, null_points=True) == (capi.MCL_ERR_INVALID_ARGUMENT, True)  # no points, but a count of them
        assert raw_search(f, fn, pts, good, 4100, null_ctx=True) == (capi.MCL_ERR_INVALID_ARGUMENT, True)
    # the candidates' entry
    lib = capi.load()
    total = C.c_uint64(77)
    ids = np.full(8, 99, dtype=np.uint64)
    poses = np.full((8, 4), 99.0)
    for params in bad:
        st = lib.mcl_global_search_candidates(f._ctx, C.byref(params), 0, 8, ids.ctypes.data_as(capi.c_u64_p), poses.ctypes.data_as(capi.c_double_p), C.byref(total))
        assert st == capi.MCL_ERR_INVALID_ARGUMENT and total.value == 77 and np.all(ids == 99) and np.all(poses == 99.0)
    good = P(1, 8, 16, 4, 0, 0)
    assert lib.mcl_global_search_candidates(f._ctx, C.byref(good), 0, 8, None, poses.ctypes.data_as(capi.c_double_p), C.byref(total)) == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.mcl_global_search_candidates(f._ctx, C.byref(good), 0, 8, ids.ctypes.data_as(capi.c_u64_p), poses.ctypes.data_as(capi.c_double_p), None) == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.mcl_global_search_candidates(None, C.byref(good), 0, 8, ids.ctypes.data_as(capi.c_u64_p), poses.ctypes.data_as(capi.c_double_p), C.byref(total)) == capi.MCL_ERR_INVALID_ARGUMENT
    assert total.value == 77 and np.all(ids == 99) and np.all(poses == 99.0)
    f.close()
    # what mcl_likelihoods refuses of the measurement: more than 4096 points on a beam context
    f = Amcl(grid, MOTION, BEAM, SMALL, seed=1)
    assert raw_search(f, "mcl_global_search", np.zeros((4097, 2)), P(1, 8, 16, 4, 0, 0), 4100) == (capi.MCL_ERR_INVALID_ARGUMENT, True)
    f.close()
    # no map
    f = Amcl(None, MOTION, LF, SMALL, seed=1)
    assert raw_search(f, "mcl_global_search", pts, P(1, 8, 16, 4, 0, 0), 4100) == (capi.MCL_ERR_NOT_READY, True)
    st = lib.mcl_global_search_candidates(f._ctx, C.byref(good), 0, 8, ids.ctypes.data_as(capi.c_u64_p), poses.ctypes.data_as(capi.c_double_p), C.byref(total))
    assert st == capi.MCL_ERR_NOT_READY and total.value == 77
    f.close()
    # other sensor models
    import os

    ndt_map = load_ndt_map_npz(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "turtlebot3_world_ndt.npz"))
    box = LandmarkMapBoundaries((-6.0, -6.0, 0.0), (6.0, 6.0, 2.0))
    landmark_map = LandmarkMap(box, [LandmarkPositionDetection((1.0, 2.0, 0.5), 0), LandmarkPositionDetection((-2.0, 1.0, 1.0), 1)])
    others = ((ndt_map, NDTModelParam2d()), (landmark_map, LandmarkModelParam(sigma_range=0.2, sigma_bearing=0.1, random_prob=1e-3)),
              (landmark_map, BearingModelParam(sigma_bearing=0.1, sensor_pose_in_robot=(0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.5))))
    for other_map, sensor in others:
        f = Amcl(other_map, MOTION, sensor, SMALL, seed=1)
        for fn in ("mcl_global_search", "mcl_global_search_pool"):
            assert raw_search(f, fn, pts, P(1, 8, 16, 4, 0, 0), 4100) == (capi.MCL_ERR_UNSUPPORTED, True), type(sensor).__name__
        st = lib.mcl_global_search_candidates(f._ctx, C.byref(good), 0, 8, ids.ctypes.data_as(capi.c_u64_p), poses.ctypes.data_as(capi.c_double_p), C.byref(total))
        assert st == capi.MCL_ERR_UNSUPPORTED and total.value == 77 and np.all(ids == 99), type(sensor).__name__
        f.close()


def test_a_map_without_a_candidate_cell_is_ok_with_no_hits():
    cells = np.full((6, 7), 100, dtype=np.int8)
    f = Amcl(OccupancyGrid(cells=cells, resolution=0.1, origin=se2_from_xytheta(0.0, 0.0, 0.0)), MOTION, LF, SMALL, seed=1)
    assert f.global_search(np.array([[1.0, 0.0]])) == [] and f.last_search_info["candidates"] == 0
    f.close()
