"""mcl_cast_rays* on the device against tests/raycast_reference.py (held to the oracle and to tests/beam_reference.py by
tests/test_raycast_reference_cpu.py): ranges, hit cells and the count of visited cells EQUAL, on every engineered family of
tests/beam_families.py, on a beam context (the packed bit maps: cast_ray_grid) and on a likelihood-field context of the same grid (the
int8 cells: cast_ray), which must also equal each other.  Then the chunking, the reach, the device form, the refusals, and the filter
left untouched."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import beam_families as fam
import raycast_reference as rc
import test_gpu_likelihoods as lk  # (its grids, scans, twins' snapshot and bare contexts)
from beluga_amd import capi, synth
from beluga_amd.amcl import (Amcl, AmclBatch, AmclParams, BeamModelParam, BearingModelParam, LandmarkMap, LandmarkModelParam, LikelihoodFieldModelParam,
                             NDTMap2d, NDTModelParam2d, OccupancyGrid, SharedMap, se2_from_xytheta)

pytestmark = pytest.mark.gpu

MOTION = lk.MOTION
LF = LikelihoodFieldModelParam(max_obstacle_distance=1.0, max_laser_distance=100.0, z_hit=0.5, z_random=0.5, sigma_hit=0.2)
POSE_COUNTS = (1, 3, 65)
SMALL = AmclParams(min_particles=8, max_particles=8)
ANGLES = np.array([0.0, 0.3, math.pi / 4, math.pi / 2, 2.0, math.pi, -2.5, -math.pi / 2, -0.4])

_filters, _references = {}, {}


def grid_of(case):
    return OccupancyGrid(cells=case["cells"], resolution=case["resolution"], origin=case["origin"])


def filters_for(case):
    """A beam and a likelihood-field filter per grid, kept for the module."""
    key = (id(case["cells"]), tuple(case["origin"]), case["resolution"])
    if key not in _filters:
        beam = BeamModelParam(*fam.ref.revealing_params(case["resolution"], 1.0))
        _filters[key] = (Amcl(grid_of(case), MOTION, beam, SMALL, seed=11), Amcl(grid_of(case), MOTION, LF, SMALL, seed=11))
    return _filters[key]


def reference_for(case):
    key = (id(case["cells"]), id(case["states"]), float(case["params"][6]), case["points"].tobytes())
    if key not in _references:
        _references[key] = rc.of_case(case)
    return _references[key]


@pytest.fixture(scope="module", autouse=True)
def _close_filters():
    yield
    for pair in _filters.values():
        for f in pair:
            f.close()
    _filters.clear()
    _references.clear()


def cast(f, poses, **how):
    ranges, hits, visited = f.cast_rays(poses, hit_cells=True, cells_visited=True, **how)
    assert ranges.shape == hits.shape == (len(poses), ranges.shape[1]) and ranges.dtype == np.float64 and hits.dtype == np.int64
    return ranges, hits, visited


def check_case(case):
    r = reference_for(case)
    max_range = float(case["params"][6])
    m = len(case["states"])
    runs = [fam.assignment(case, n) for n in POSE_COUNTS] + [np.arange(m)]  # (and every state of the case once)
    for idx in runs:
        want = r["ranges"][idx], r["hit_cells"][idx], int(r["visited"][idx].sum())
        got = [cast(f, case["states"][idx], points=case["points"], max_range=max_range) for f in filters_for(case)]
        for kind, (ranges, hits, visited) in zip(("beam", "lf"), got):
            print("cast_rays %s %s n=%d B=%d cells=%d (want %d)" % (case["targets"], kind, len(idx), len(case["points"]), visited, want[2]))
            assert np.array_equal(lk.bits(ranges), lk.bits(want[0])), (case["targets"], kind, len(idx))
            assert np.array_equal(hits, want[1]), (case["targets"], kind, len(idx))
            assert visited == want[2], (case["targets"], kind, len(idx), visited, want[2])
        assert np.array_equal(lk.bits(got[0][0]), lk.bits(got[1][0])) and np.array_equal(got[0][1], got[1][1]) and got[0][2] == got[1][2]


# ---- 1. the families -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in fam.FAMILIES if n != "beam_counts"))
def test_every_family_equals_the_reference_on_both_walks(name):
    for case in fam.FAMILIES[name]():
        check_case(case)


def test_every_beam_count_and_a_table_beyond_the_workgroup():
    """B = 1, 7, 8, 9, 63, 64, 65, 129: a table shorter than the workgroup lies in LDS and a wave's lanes cross poses; 4097 bearings - more
    than mcl_likelihoods takes on a beam context - are read from memory, a bearing per lane."""
    scan, many = fam.beam_counts()
    for B in fam.BEAM_COUNTS:
        check_case(fam.prefix(scan, B))
    check_case(fam.prefix(many, 4097))
    check_case(fam.prefix(many, 257))  # the memory path where a workgroup crosses a pose boundary in its last lane


# ---- 2. the reach bound -----------------------------------------------------------------------------------------------------------------
def test_a_reach_one_cell_below_the_bound_is_cast_and_the_bound_is_refused():
    case = fam.closed_form_thresholds()[0]
    assert case["resolution"] == fam.POW
    states, bearings = case["states"][:3], rc.bearings_of_angles(ANGLES)
    below, at = (2.0 ** 27 - 3.0) * fam.POW, (2.0 ** 27 - 2.0) * fam.POW
    want = rc.cast_rays(case["cells"], fam.POW, case["origin"], states, bearings, below)
    for f in filters_for(case):
        ranges, hits, visited = cast(f, states, bearings=bearings, max_range=below)
        assert np.array_equal(lk.bits(ranges), lk.bits(want["ranges"])) and np.array_equal(hits, want["hit_cells"]) and visited == want["cells_visited"]
        status, outs = raw(f, states, bearings, at)
        assert status == capi.MCL_ERR_INVALID_ARGUMENT and untouched(outs)


# ---- 3. chunking ------------------------------------------------------------------------------------------------------------------------
def test_the_result_does_not_depend_on_cast_chunk():
    case = fam.prefix(fam.beam_counts()[0], 129)
    idx = fam.assignment(case, 65)
    r = reference_for(case)
    for f in filters_for(case):
        results = []
        for chunk in (0, 100, 129 * 3 + 1, 1 << 22):  # the minimum (64), chunks that split a pose's 129 bearings, the default: one chunk
            f.set_option("cast_chunk", chunk)
            results.append(cast(f, case["states"][idx], points=case["points"], max_range=float(case["params"][6])))
        f.set_option("cast_chunk", 1 << 22)
        for ranges, hits, visited in results:
            assert np.array_equal(lk.bits(ranges), lk.bits(r["ranges"][idx])) and np.array_equal(hits, r["hit_cells"][idx])
            assert visited == int(r["visited"][idx].sum())


# ---- 4. out of reach ----------------------------------------------------------------------------------------------------------------------
def test_poses_out_of_reach_hit_nothing_and_visit_nothing():
    case = fam.closed_form_thresholds()[0]  # (a resolution with an exact reciprocal)
    if not np.array_equal(case["origin"], fam.IDENTITY):
        case = dict(case, origin=fam.IDENTITY)
    res, bearings = case["resolution"], rc.bearings_of_angles(ANGLES)
    edge = 2.0 ** 30 * res
    poses = np.array([[1.0, 0.0, 1e12, 0.0], [0.0, 1.0, -1e12, 1e12], [1.0, 0.0, edge, 0.5], [1.0, 0.0, -edge, 0.5], [1.0, 0.0, 0.5, edge],
                      [1.0, 0.0, 0.5, -edge], [1.0, 0.0, edge - res, 0.5], [1.0, 0.0, 0.5, 0.5]])
    want = rc.cast_rays(case["cells"], res, case["origin"], poses, bearings, 3.0)
    assert (want["ranges"][:7] == 3.0).all() and (want["hit_cells"][:7] == -1).all() and want["visited"][:7].sum() == 0
    for f in (Amcl(grid_of(case), MOTION, BeamModelParam(*fam.ref.revealing_params(res, 1.0)), SMALL, seed=1), Amcl(grid_of(case), MOTION, LF, SMALL, seed=1)):
        ranges, hits, visited = cast(f, poses, bearings=bearings, max_range=3.0)
        assert np.array_equal(lk.bits(ranges), lk.bits(want["ranges"])) and np.array_equal(hits, want["hit_cells"]) and visited == want["cells_visited"]
        # a bearing that is no unit vector: a line of 2^27 cells is out of reach, its neighbour is cast
        long = np.array([[2.0 ** 27, 0.0], [1.0, 0.0]])
        w = rc.cast_rays(case["cells"], res, case["origin"], poses[7:], long, res)
        ranges, hits, visited = cast(f, poses[7:], bearings=long, max_range=res)
        assert np.array_equal(lk.bits(ranges), lk.bits(w["ranges"])) and np.array_equal(hits, w["hit_cells"]) and visited == w["cells_visited"]
        assert hits[0, 0] == -1
        f.close()


# ---- 5. the device form ---------------------------------------------------------------------------------------------------------------------
def test_device_form_gives_the_host_forms_bits():
    import torch

    case = fam.prefix(fam.beam_counts()[0], 65)
    max_range = float(case["params"][6])
    for f in filters_for(case):
        for n in (1, 65, 1030):
            states = case["states"][fam.assignment(case, n)]
            host = cast(f, states, points=case["points"], max_range=max_range)
            d_poses = torch.from_numpy(np.ascontiguousarray(states)).to("cuda:0")
            ranges, hits, visited = f.cast_rays_device(d_poses, points=case["points"], max_range=max_range, hit_cells=True, cells_visited=True)
            assert ranges.dtype == torch.float64 and hits.dtype == torch.int64 and tuple(ranges.shape) == (n, 65)
            assert np.array_equal(lk.bits(ranges.cpu().numpy()), lk.bits(host[0])) and np.array_equal(hits.cpu().numpy(), host[1]) and visited == host[2]
            alone = f.cast_rays_device(d_poses, points=case["points"], max_range=max_range)  # no hit cells, no count
            assert np.array_equal(lk.bits(alone.cpu().numpy()), lk.bits(host[0]))


@pytest.mark.parametrize("sensor", [lk.LF, lk.BEAM], ids=["lf", "beam"])
def test_device_form_called_again_while_the_first_call_is_in_flight(sensor):
    """Two calls in a row with nothing waited for between them: the second, of a longer bearing table, writes the staging memory again
    and makes it grow.  Each output is what the host form gives for its table on a twin."""
    import torch

    grid, poses = lk.reuse_grid(), lk.reuse_poses()
    tables = [np.array([[1.0, 0.0], [0.6, 0.8]]), np.array([[0.0, -1.0], [-0.8, 0.6], [-1.0, 0.0]])]
    f = Amcl(grid, MOTION, sensor, AmclParams(max_particles=64), seed=1)
    twin = Amcl(grid, MOTION, sensor, AmclParams(max_particles=64), seed=1)
    d_poses = torch.from_numpy(poses).to("cuda:0")
    outs = [f.cast_rays_device(d_poses, bearings=table, max_range=3.0, synchronize=False) for table in tables]
    f.sync()
    for got, table in zip(outs, tables):
        host = twin.cast_rays(poses, bearings=table, max_range=3.0)
        assert tuple(got.shape) == (64, len(table)) and np.array_equal(lk.bits(got.cpu().numpy()), lk.bits(host))
        assert np.unique(host).size > 8  # (walls at many distances: no constant answer passes)
    f.close()
    twin.close()


# ---- 6. the filter is untouched ---------------------------------------------------------------------------------------------------------------
PROBE_ANGLES = np.linspace(-math.pi, math.pi, 33, endpoint=False)


def probe_of(truth):
    return lk.poses_around(truth, 6, seed=8)


def ask(f, probe, max_range=6.0):
    return cast(f, probe, angles=PROBE_ANGLES, max_range=max_range)


def run_twins(asked, twin, truth, scan_of, probe, before_cycle=None, cycles=5, step_of=None):
    """Five update cycles on both; `asked` casts rays before the first and between every two.  Returns each call's outputs."""
    answers = [ask(asked, probe)]
    pose, odom = truth, (0.0, 0.0, 0.0)
    for c in range(cycles):
        if before_cycle:
            before_cycle(c)
        pose, odom = synth.odometry_step(pose, 0.3, 0.05), synth.odometry_step(odom, 0.3, 0.05)
        pts = scan_of(pose, c)
        a, b = asked.update(se2_from_xytheta(*odom), pts), twin.update(se2_from_xytheta(*odom), pts)
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(lk.bits(a[0]), lk.bits(b[0])) and np.array_equal(lk.bits(a[1]), lk.bits(b[1])), c
        assert lk.snapshot(asked) == lk.snapshot(twin), c
        answers.append(ask(asked, probe))
        assert lk.snapshot(asked) == lk.snapshot(twin), c  # (the call itself moved nothing either)
    return answers


def same_answer(got, grid, probe, max_range=6.0):
    want = rc.cast_rays(grid.cells, grid.resolution, grid.origin, probe, rc.bearings_of_angles(PROBE_ANGLES), max_range)
    return np.array_equal(lk.bits(got[0]), lk.bits(want["ranges"])) and np.array_equal(got[1], want["hit_cells"]) and got[2] == want["cells_visited"]


def test_untouched_lf_kld_adaptive(lk_world):
    grid, truth = lk_world
    params = AmclParams(min_particles=500, max_particles=20_000, update_min_d=0.0, update_min_a=0.0, resample_interval=1)
    pair = [Amcl(grid, MOTION, lk.LF, params, seed=42) for _ in range(2)]
    for f in pair:
        f.initialize(truth, lk.COV)
    probe = probe_of(truth)
    answers = run_twins(pair[0], pair[1], truth, lk.lf_scan(grid, 65), probe)
    assert pair[0].num_particles() != 20_000  # (the set's size did change)
    assert same_answer(answers[0], grid, probe) and all(np.array_equal(a[0], answers[0][0]) and a[2] == answers[0][2] for a in answers)
    for f in pair:
        f.close()


def test_untouched_beam_filter_and_its_cell_counter(lk_world):
    grid, truth = lk_world
    params = AmclParams(min_particles=300, max_particles=1000, update_min_d=0.0, update_min_a=0.0, resample_interval=1)
    pair = [Amcl(grid, MOTION, lk.BEAM, params, seed=5) for _ in range(2)]
    for f in pair:
        f.initialize(truth, lk.COV)
        f.beam_cells_visited(reset=True)
    probe = probe_of(truth)
    answers = run_twins(pair[0], pair[1], truth, lk.lf_scan(grid, 33), probe)
    assert pair[0].beam_cells_visited(reset=False) == pair[1].beam_cells_visited(reset=False) > 0  # the cycle's own count: the calls added nothing
    assert same_answer(answers[-1], grid, probe)
    for f in pair:
        f.close()


def test_untouched_on_a_shared_map_and_across_an_async_map_swap(lk_world):
    grid, truth = lk_world
    grid_b = lk.rooms_grid(400, 9)
    params = AmclParams(min_particles=300, max_particles=1000, update_min_d=0.0, update_min_a=0.0, resample_interval=1)
    shared = SharedMap(grid, lk.LF)
    on_shared = [Amcl(grid, MOTION, lk.LF, params, seed=7) for _ in range(2)]
    for f in on_shared:
        f.use_map(shared)
        f.initialize(truth, lk.COV)
    probe = probe_of(truth)
    answers = run_twins(on_shared[0], on_shared[1], truth, lk.lf_scan(grid, 33), probe)
    assert same_answer(answers[2], grid, probe)
    for f in on_shared:
        f.close()
    shared.close()
    swapping = [Amcl(grid, MOTION, lk.LF, params, seed=7) for _ in range(2)]
    for f in swapping:
        f.initialize(truth, lk.COV)

    def before_cycle(c):
        if c == 1:
            for f in swapping:
                f.update_map_async(grid_b)
        if c == 3:
            for f in swapping:
                f.map_commit(wait=True)

    answers = run_twins(swapping[0], swapping[1], truth, lk.lf_scan(grid, 33), probe, before_cycle)
    # the rays follow the map the context reads: the old one while the new one is pending, the new one from its swap on
    for c in range(5):
        assert same_answer(answers[c + 1], grid if c < 3 else grid_b, probe), c
    assert not same_answer(answers[5], grid, probe)
    for f in swapping:
        f.close()


def test_untouched_member_of_a_batch(lk_world):
    grid, truth = lk_world
    params = AmclParams(min_particles=300, max_particles=600, update_min_d=0.0, update_min_a=0.0, resample_interval=1)
    specs = [dict(grid=grid, motion=MOTION, sensor=lk.LF, params=params, seed=20 + k) for k in range(3)]
    fleets = [AmclBatch(specs) for _ in range(2)]
    for fleet in fleets:
        for m in fleet.members:
            m.initialize(truth, lk.COV)
    probe = probe_of(truth)
    asked = fleets[0].members[1]
    ask(asked, probe)
    pose, odom = truth, (0.0, 0.0, 0.0)
    for c in range(5):
        pose, odom = synth.odometry_step(pose, 0.3, 0.05), synth.odometry_step(odom, 0.3, 0.05)
        pts = lk.make_scan(grid, pose, 33, seed=c)
        results = [fleet.update([se2_from_xytheta(*odom)] * 3, [pts] * 3) for fleet in fleets]
        for a, b in zip(*results):
            assert (a is None) == (b is None)
            if a is not None:
                assert np.array_equal(lk.bits(a[0]), lk.bits(b[0])) and np.array_equal(lk.bits(a[1]), lk.bits(b[1])), c
        for a, b in zip(fleets[0].members, fleets[1].members):
            assert lk.snapshot(a) == lk.snapshot(b), c
        assert fleets[0].last_infos == fleets[1].last_infos
        assert all(fleets[0].counter(name) == fleets[1].counter(name) for name in lk.BATCH_COUNTERS), c
        got = ask(asked, probe)
        if c == 4:
            assert same_answer(got, grid, probe)
    for fleet in fleets:
        fleet.close()


@pytest.fixture(scope="module")
def lk_world():
    grid = lk.rooms_grid()
    truth = synth.find_free_pose(grid.cells, grid.resolution, (grid.origin[2], grid.origin[3]), seed=2, clearance_cells=6)
    return grid, truth


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
SENTINEL, HIT_SENTINEL, COUNT_SENTINEL = -12345.0, -777, 424242


def raw(f, poses, bearings, max_range, null=(), n=None, B=None):
    """A raw call with the outputs filled with sentinels: (status, (ranges, hit cells, count))."""
    lib = capi.load()
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4)
    bearings = np.ascontiguousarray(bearings, dtype=np.float64).reshape(-1, 2)
    n, B = len(poses) if n is None else n, len(bearings) if B is None else B
    ranges = np.full(max(len(poses) * len(bearings), 1), SENTINEL)
    hits = np.full(max(len(poses) * len(bearings), 1), HIT_SENTINEL, dtype=np.int64)
    count = C.c_uint64(COUNT_SENTINEL)
    status = lib.mcl_cast_rays(f._ctx, None if "poses" in null else poses.ctypes.data_as(capi.c_double_p), n,
                               None if "bearings" in null else bearings.ctypes.data_as(capi.c_double_p), B, max_range,
                               None if "ranges" in null else ranges.ctypes.data_as(capi.c_double_p), hits.ctypes.data_as(capi.c_i64_p), C.byref(count))
    return status, (ranges, hits, count.value)


def untouched(outs, count=COUNT_SENTINEL):
    return (outs[0] == SENTINEL).all() and (outs[1] == HIT_SENTINEL).all() and outs[2] == count


def test_refusals_leave_the_outputs_as_they_were(lk_world):
    import torch

    grid, truth = lk_world
    poses, bearings = probe_of(truth), rc.bearings_of_angles(ANGLES)
    lf = Amcl(grid, MOTION, lk.LF, AmclParams(max_particles=64), seed=1)
    beam = Amcl(grid, MOTION, lk.BEAM, AmclParams(max_particles=64), seed=1)
    ndt = Amcl(NDTMap2d(np.array([[0, 0]], dtype=np.int32), np.array([[0.5, 0.5]]), np.array([[[0.1, 0.0], [0.0, 0.1]]]), 1.0), MOTION,
               NDTModelParam2d(), AmclParams(max_particles=64), seed=1)
    landmark_map = LandmarkMap((np.array([[1.0, 1.0, 0.0], [2.0, 0.0, 0.0]]), np.array([0, 1], dtype=np.uint32)))
    lm = Amcl(landmark_map, MOTION, LandmarkModelParam(0.3, 0.2, 0.1), AmclParams(max_particles=64), seed=1)
    br = Amcl(landmark_map, MOTION, BearingModelParam(0.2, (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.5)), AmclParams(max_particles=64), seed=1)
    no_map = AmclBatch([dict(grid=None, motion=MOTION, sensor=lk.LF, params=AmclParams(min_particles=100, max_particles=100))])
    U, A, R = capi.MCL_ERR_UNSUPPORTED, capi.MCL_ERR_INVALID_ARGUMENT, capi.MCL_ERR_NOT_READY

    def refused(result, want):
        status, outs = result
        assert status == want and untouched(outs), (status, want)

    for f in (ndt, lm, br):
        refused(raw(f, poses, bearings, 5.0), U)
    refused(raw(no_map.members[0], poses, bearings, 5.0), R)
    for f in (lf, beam):
        for which in ("poses", "bearings", "ranges"):
            refused(raw(f, poses, bearings, 5.0, null=(which,)), A)
        for bad in (np.nan, np.inf, -np.inf):
            broken = poses.copy()
            broken[3, 2] = bad
            refused(raw(f, broken, bearings, 5.0), A)
            broken = bearings.copy()
            broken[4, 1] = bad
            refused(raw(f, poses, broken, 5.0), A)
        for bad in (np.nan, np.inf, -np.inf, 0.0, -1.0, 2.0 ** 27 * grid.resolution):
            refused(raw(f, poses, bearings, bad), A)
            refused(raw(f, poses, bearings, bad, n=0), A)  # max_range is checked whatever the counts
        # zero counts: MCL_OK, nothing written but the count
        for n, B in ((0, None), (None, 0), (0, 0)):
            status, outs = raw(f, poses, bearings, 5.0, null=("poses", "bearings", "ranges"), n=n, B=B)
            assert status == capi.MCL_OK and untouched(outs, count=0)
        # the facade refuses what it can before the call
        with pytest.raises(ValueError):
            f.cast_rays(poses, bearings=bearings, angles=ANGLES, max_range=5.0)
        with pytest.raises(ValueError):
            f.cast_rays(poses, max_range=5.0)
    with pytest.raises(ValueError):
        lf.cast_rays(poses, angles=ANGLES)  # only a beam filter has a max_range of its own
    assert beam.cast_rays(poses, angles=ANGLES).shape == (len(poses), len(ANGLES))
    # the device form: the device memory keeps the sentinel
    lib = capi.load()
    d_poses = torch.from_numpy(poses).to("cuda:0")
    d_ranges = torch.full((len(poses) * len(bearings),), SENTINEL, dtype=torch.float64, device="cuda:0")
    d_hits = torch.full((len(poses) * len(bearings),), HIT_SENTINEL, dtype=torch.int64, device="cuda:0")

    def device_form(f, table, max_range):
        table = np.ascontiguousarray(table, dtype=np.float64)
        count = C.c_uint64(COUNT_SENTINEL)
        status = lib.mcl_cast_rays_device(f._ctx, d_poses.data_ptr(), len(poses), table.ctypes.data_as(capi.c_double_p), len(table), max_range,
                                          d_ranges.data_ptr(), d_hits.data_ptr(), C.byref(count))
        torch.cuda.synchronize()
        return status, (d_ranges.cpu().numpy(), d_hits.cpu().numpy(), count.value)

    for f in (ndt, lm, br):
        refused(device_form(f, bearings, 5.0), U)
    refused(device_form(no_map.members[0], bearings, 5.0), R)
    broken = bearings.copy()
    broken[0, 0] = np.nan
    refused(device_form(lf, broken, 5.0), A)
    refused(device_form(beam, bearings, -1.0), A)
    for f in (lf, beam, ndt, lm, br):
        f.close()
    no_map.close()


# ---- 8. the expected scan ------------------------------------------------------------------------------------------------------------------------
def test_expected_scan_on_the_turtlebot_map():
    z = np.load(os.path.join(lk.GOLDEN, "turtlebot3_world_grid.npz"))
    ox, oy, ot = z["origin_xytheta"]
    grid = OccupancyGrid(cells=z["cells"], resolution=float(z["resolution"]), origin=se2_from_xytheta(ox, oy, ot))
    x, y, theta = synth.find_free_pose(grid.cells, grid.resolution, (grid.origin[2], grid.origin[3]), seed=2, clearance_cells=4)
    angles = np.deg2rad(np.arange(360.0))
    pose = np.array([[math.cos(theta), math.sin(theta), x, y]])
    want = rc.cast_rays(grid.cells, grid.resolution, grid.origin, pose, rc.bearings_of_angles(angles), 3.5)
    assert (want["hit_cells"] >= 0).sum() > 100  # (a room: most rays end on a wall)
    for sensor in (lk.LF, BeamModelParam(0.5, 0.05, 0.05, 0.5, 0.2, 0.1, 3.5)):
        f = Amcl(grid, MOTION, sensor, AmclParams(max_particles=64), seed=1)
        got = f.expected_scan((x, y, theta), angles, 3.5)
        assert got.shape == (360,) and np.array_equal(lk.bits(got), lk.bits(want["ranges"][0]))
        f.close()
