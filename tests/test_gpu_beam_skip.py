"""Beam skipping on the device (include/beluga_mcl.h "Beam skipping"), held to tests/beam_skip_reference.py:

  * the counts of mcl_beam_agreement equal agreement_counts - integers, `==` - on the engineered end-points of tests/lf_families.py,
    on a field where a wrong cell shows (lf_reference.revealing_field with the level set inside its palette: a neighbouring cell is on
    the other side of it more often than not), for every set size at which the kernel's geometry changes and for a scan one beam longer
    than a pass of the kernel (PASS + 1); on private, shared and device-built maps, and behind a second map;
  * the call leaves the filter untouched (a twin that never made it is the comparison);
  * an enabled mcl_reweight is the disabled one of the kept points, bit for bit, and so is a whole cycle; the counts a cycle reports
    are those of the set its propagation left (a third context repeats that propagation);
  * skipping does what it is for: the beams an unmapped person shortens are voted out and the weights are those of the clean beams; a
    cloud in the wrong place uses the whole scan;
  * off is off; what is refused; a batch member with skipping on runs its lone cycle.

All exact comparisons use the level the LIBRARY reports (held to one float ulp of numpy's), so exp's last bit cannot blur a count.
"""
import ctypes as C
import os

import numpy as np
import pytest

import beam_skip_reference as bref
import lf_families as fam
import lf_reference as ref
from beluga_amd import capi, synth
from beluga_amd.amcl import (Amcl, AmclBatch, AmclParams, BeamModelParam, DifferentialDriveModelParam, LikelihoodFieldModelParam,
                             LikelihoodFieldProbModelParam, OccupancyGrid, SharedMap, se2_from_xytheta)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
LF_ARGS = (2.0, 100.0, 0.5, 0.5, 0.2)  # max_obstacle_distance, max_laser_distance, z_hit, z_random, sigma_hit
LF = LikelihoodFieldModelParam(*LF_ARGS, True)
LF_PROB = LikelihoodFieldProbModelParam(*LF_ARGS, True)
PASS = 4096  # kBeamSkipPass (csrc/kernels.h): beams of one launch of the count
# every size at which the count's geometry changes: one lane, a wave less / exactly / more than one, more than a workgroup, the small
# cycle's limit and one above, and one above lf_small_particles - more workgroups than the grid's cap of 1024 would need 262 144
SIZES = (1, 63, 64, 65, 257, 4096, 4097, 70_001)
# The revealing field's 17 values are 0.2 .. 1.2 in steps of 1/16; at distance 0.17 m the level is ~0.70: eight values above, nine below.
REVEALING_DISTANCE = 0.17
COUNTERS = ("lf_fast_launches", "lf_patch_launches", "lf_queue_launches", "lf_beams_launches", "lf_far_launches", "lf_far_beams_launches",
            "small_tail_launches", "estimate_repivots", "noise_ahead_used", "order_ahead_used", "order_ahead_missed", "field_pose_rebuilds",
            "host_cycles", "cluster_cells", "beam_skip_launches", "beam_skip_used_all")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def library_level(f):
    return np.float32(f.beam_skip_result()["level"])


def reference_level(distance):
    return bref.level(LF_ARGS[2], LF_ARGS[3], LF_ARGS[4], LF_ARGS[1], distance)


def check_level(f, distance):
    got, want = library_level(f), reference_level(distance)
    assert abs(int(got.view(np.uint32)) - int(want.view(np.uint32))) <= 1, (got, want)
    return got


# ---- 1. the counts, exact ---------------------------------------------------------------------------------------------------------------
_filters = {}


def family_filter(case, capacity, prob):
    key = (case["shape"], case["resolution"], tuple(case["origin"]), capacity, prob)
    if key not in _filters:
        H, W = case["shape"]
        grid = OccupancyGrid(cells=np.zeros((H, W), dtype=np.int8), resolution=case["resolution"], origin=case["origin"])
        f = Amcl(grid, MOTION, LF_PROB if prob else LF, AmclParams(min_particles=capacity, max_particles=capacity), seed=11)
        f.set_likelihood_field(ref.revealing_field(H, W, "palette"))
        f.set_beam_skip(False, distance=REVEALING_DISTANCE)
        _filters[key] = f
    return _filters[key]


@pytest.fixture(scope="module", autouse=True)
def _close_filters():
    yield
    for f in _filters.values():
        f.close()
    _filters.clear()


def check_counts(case, points, n, prob=False):
    H, W = case["shape"]
    f = family_filter(case, max(n, 4097), prob)
    level = check_level(f, REVEALING_DISTANCE)
    assert 0.6 < level < 0.8
    states = case["states"][np.arange(n) % len(case["states"])]
    f.set_particles(states, np.ones(n))
    got = f.beam_agreement(points)
    want = bref.agreement_counts(ref.revealing_field(H, W, "palette"), level, case["resolution"], case["origin"], states, points)
    assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), want), (case["targets"], n, np.flatnonzero(got != want)[:8])
    return want


@pytest.mark.parametrize("family", ["ulp_straddle", "trigger_ring", "borders", "small_grids", "beam_counts", "no_cell"])
@pytest.mark.parametrize("prob", [False, True])
def test_counts_are_exact_on_the_engineered_end_points(family, prob):
    voted = 0
    for case in fam.FAMILIES[family]():
        points = case["points"][:257]
        for n in (len(case["states"]), 65):
            want = check_counts(case, points, n, prob)
            voted += int((want > 0).sum())
    if family != "no_cell":
        assert voted > 0  # (the level cuts the palette: some beams agree, and - checked by the equality - some do not)


@pytest.mark.parametrize("n", SIZES)
def test_counts_are_exact_at_every_set_size(n):
    case = fam.beam_counts()[0]
    want = check_counts(case, case["points"][:129], n)
    assert 0 < want.max() <= n and want.min() < n


def test_counts_of_a_scan_one_beam_longer_than_a_pass():
    case = fam.beam_counts()[0]
    points = np.tile(case["points"], (4, 1))[:PASS + 1]
    assert len(points) == PASS + 1
    want = check_counts(case, points, 257)
    assert want[PASS] == want[PASS % len(case["points"])]  # (the beam of the second pass is a repeat of an early one)
    check_counts(case, points[:PASS], 65)


def test_no_points_and_points_without_a_cell():
    case = fam.no_cell()[-1]  # a scan of nothing but points without a cell
    f = family_filter(case, 4097, False)
    f.set_particles(case["states"], np.ones(len(case["states"])))
    before = f.counter("beam_agreement_calls")
    assert len(f.beam_agreement(np.zeros((0, 2)))) == 0
    assert f.counter("beam_agreement_calls") == before
    assert not f.beam_agreement(case["points"]).any()


def turtlebot():
    z = np.load(os.path.join(GOLDEN, "turtlebot3_world_grid.npz"))
    ox, oy, ot = z["origin_xytheta"]
    return OccupancyGrid(cells=z["cells"], resolution=float(z["resolution"]), origin=se2_from_xytheta(ox, oy, ot))


def turtlebot_scene(beams=180, seed=2):
    grid = turtlebot()
    truth = synth.find_free_pose(grid.cells, grid.resolution, (grid.origin[2], grid.origin[3]), seed=seed, clearance_cells=4)
    angles = synth.lidar_angles(beams, 270.0)
    ranges = synth.cast_scan(grid.cells, grid.resolution, (grid.origin[2], grid.origin[3]), truth, angles, 3.5)
    return grid, truth, angles, ranges


def test_private_shared_and_device_built_maps_and_a_second_map():
    grid, truth, angles, ranges = turtlebot_scene()
    points = synth.scan_points(ranges, angles)
    n = 4097
    states = synth.normal_particles(n, truth, (0.3, 0.3, 0.3), seed=3)
    prm = AmclParams(min_particles=n, max_particles=n)
    shared = SharedMap(grid, LF)
    private, attached = (Amcl(grid, MOTION, LF, prm, seed=1) for _ in range(2))
    device_built = Amcl(grid, MOTION, LF, prm, seed=1, options={"field_build": 1})
    attached.use_map(shared)
    assert attached.counter("map_shared") == 1 and device_built.counter("field_built_on_device") == 1
    counts = []
    for f in (private, attached, device_built):
        f.set_particles(states, np.ones(n))
        level = check_level(f, 0.5)
        got = f.beam_agreement(points)
        want = bref.agreement_counts(f.likelihood_field(), level, grid.resolution, grid.origin, states, points)
        assert np.array_equal(got.astype(np.int64), want)
        counts.append(got)
    assert np.array_equal(counts[0], counts[1])
    if np.array_equal(private.likelihood_field(), device_built.likelihood_field()):
        assert np.array_equal(counts[0], counts[2])
    assert 0 < counts[0].max() and counts[0].min() < n
    # a second map: the counts follow it
    other = OccupancyGrid(cells=np.ascontiguousarray(grid.cells[::-1, ::-1]), resolution=grid.resolution, origin=grid.origin)
    private.update_map(other)
    got = private.beam_agreement(points)
    want = bref.agreement_counts(private.likelihood_field(), library_level(private), grid.resolution, grid.origin, states, points)
    assert np.array_equal(got.astype(np.int64), want) and not np.array_equal(got, counts[0])
    for f in (private, attached, device_built):
        f.close()
    shared.close()


# ---- 2. the filter is untouched -----------------------------------------------------------------------------------------------------------
def snapshot(f):
    states, weights = f.particles()
    return states, weights, {c: f.counter(c) for c in COUNTERS}


def test_beam_agreement_leaves_the_filter_untouched():
    grid, truth, angles, ranges = turtlebot_scene()
    points = synth.scan_points(ranges, angles)
    prm = AmclParams(min_particles=500, max_particles=2000, update_min_d=0.0, update_min_a=0.0)
    asked, twin = (Amcl(grid, MOTION, LF, prm, seed=5) for _ in range(2))
    pose = truth
    for f in (asked, twin):
        f.initialize(truth, np.diag([0.05, 0.05, 0.02]))
    for k in range(4):
        pose = synth.odometry_step(pose, 0.05, 0.02)
        ctrl = se2_from_xytheta(*pose)
        results = [f.update(ctrl, points) for f in (asked, twin)]
        assert same_bits(results[0][0], results[1][0]) and same_bits(results[0][1], results[1][1]) and asked.last_info == twin.last_info
        a, b = snapshot(asked), snapshot(twin)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and a[2] == b[2]
        calls = asked.counter("beam_agreement_calls")
        asked.beam_agreement(points)
        asked.beam_agreement(points[:7])
        assert asked.counter("beam_agreement_calls") == calls + 2 and twin.counter("beam_agreement_calls") == 0
        a = snapshot(asked)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and a[2] == b[2]
    for f in (asked, twin):
        f.close()


# ---- 3. the point of it: a room, a person ----------------------------------------------------------------------------------------------------
def room_scene(beams=180):
    """A 10 m x 10 m room with walls two cells thick, the robot near its middle, a scan cast from there; a contiguous sixth of the
    beams pulled in to 40 % of their range: an unmapped person.  Those end-points are metres from any wall."""
    cells = np.zeros((200, 200), dtype=np.int8)
    cells[:2, :] = cells[-2:, :] = cells[:, :2] = cells[:, -2:] = 100
    grid = OccupancyGrid(cells=cells, resolution=0.05, origin=se2_from_xytheta(0.0, 0.0, 0.0))
    truth = (5.2, 4.9, 0.3)
    angles = synth.lidar_angles(beams, 270.0)
    ranges = synth.cast_scan(cells, 0.05, (0.0, 0.0), truth, angles, 12.0)
    pulled = np.zeros(beams, dtype=bool)
    pulled[beams // 3: beams // 3 + beams // 6] = True
    seen = np.where(pulled, 0.4 * ranges, ranges)
    return grid, truth, synth.scan_points(seen, angles), pulled


WRONG_PLACE = (2.6, 2.4, 0.8)  # where the same scan fits nothing: see test_skipping_votes_out_what_the_map_does_not_know


def test_skipping_votes_out_what_the_map_does_not_know():
    grid, truth, points, pulled = room_scene()
    n = 2000
    prm = AmclParams(min_particles=n, max_particles=n)
    on, off = (Amcl(grid, MOTION, LF, prm, seed=9) for _ in range(2))
    on.set_beam_skip(True)
    params = on.beam_skip()
    assert params == dict(bref.DEFAULTS, enabled=True)
    field = on.likelihood_field()
    level = check_level(on, 0.5)
    assert np.array_equal(field, off.likelihood_field())
    used_all_before = on.counter("beam_skip_used_all")

    # the cloud around the true pose: exactly the person's beams go
    states = synth.normal_particles(n, truth, (0.05, 0.05, 0.02), seed=4)
    w0 = np.random.Generator(np.random.MT19937(6)).uniform(0.5, 1.5, n)
    want_counts = bref.agreement_counts(field, level, grid.resolution, grid.origin, states, points)
    want_kept, want_skipped, want_all = bref.decide(want_counts, n, len(points), params)
    assert np.array_equal(~want_kept, pulled) and not want_all  # (the scene does what it was built for, by the reference alone)
    for f in (on, off):
        f.set_particles(states, w0)
    launches = on.counter("beam_skip_launches")
    on.reweight(points)
    off.reweight(points[~pulled])
    r = on.beam_skip_result()
    assert r["valid"] and not r["used_all"] and r["num_beams"] == len(points) and r["num_particles"] == n and r["num_skipped"] == want_skipped
    assert np.array_equal(r["counts"].astype(np.int64), want_counts) and np.array_equal(r["kept"], want_kept)
    assert np.array_equal(~r["kept"], pulled)
    assert same_bits(on.particles()[1], off.particles()[1])
    assert on.counter("beam_skip_launches") == launches + 1 and on.counter("beam_skip_used_all") == used_all_before
    # (and the person's beams did matter: the weights of the whole scan are others)
    off.set_particles(states, w0)
    off.reweight(points)
    assert not same_bits(on.particles()[1], off.particles()[1])

    # the cloud in the wrong place: at least 90 % of the beams disagree with it, and the whole scan has its say
    states = synth.normal_particles(n, WRONG_PLACE, (0.05, 0.05, 0.02), seed=5)
    want_counts = bref.agreement_counts(field, level, grid.resolution, grid.origin, states, points)
    want_kept, want_skipped, want_all = bref.decide(want_counts, n, len(points), params)
    assert want_skipped >= 0.9 * len(points) and want_all  # (such a spot, by the reference alone)
    for f in (on, off):
        f.set_particles(states, w0)
    on.reweight(points)
    off.reweight(points)
    r = on.beam_skip_result()
    assert r["valid"] and r["used_all"] and r["num_skipped"] == want_skipped and np.array_equal(r["kept"], want_kept)
    assert np.array_equal(r["counts"].astype(np.int64), want_counts)
    assert same_bits(on.particles()[1], off.particles()[1])
    assert on.counter("beam_skip_used_all") == used_all_before + 1
    for f in (on, off):
        f.close()


# ---- 4. stage level and whole cycles, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2000, 5000, 70_000])  # the small cycle's size, a medium set, the ordered path
@pytest.mark.parametrize("prob", [False, True])
def test_an_enabled_reweight_is_the_reweight_of_the_kept_points(n, prob):
    grid, truth, points, pulled = room_scene()
    prm = AmclParams(min_particles=n, max_particles=n)
    a, b = (Amcl(grid, MOTION, LF_PROB if prob else LF, prm, seed=21) for _ in range(2))
    a.set_beam_skip(True)
    states = synth.normal_particles(n, truth, (0.05, 0.05, 0.02), seed=8)
    pose, prev = se2_from_xytheta(0.1, 0.0, 0.01), se2_from_xytheta(0.0, 0.0, 0.0)
    for step in (1, 2):  # (the second reweight meets weights that are not 1 and field-frame poses a propagation wrote)
        for f in (a, b):
            if step == 1:
                f.set_particles(states, np.ones(n))
            f.propagate(pose, prev, step)
        a.reweight(points)
        counts = b.beam_agreement(points)
        kept, skipped, used_all = bref.decide(counts, n, len(points), a.beam_skip())
        assert 0 < skipped < len(points) and not used_all
        b.reweight(points if used_all else points[kept])
        r = a.beam_skip_result()
        assert np.array_equal(r["counts"], counts) and np.array_equal(r["kept"], kept) and r["num_skipped"] == skipped
        sa, sb = a.particles(), b.particles()
        assert same_bits(sa[0], sb[0]) and same_bits(sa[1], sb[1])
    for f in (a, b):
        f.close()


@pytest.mark.parametrize("prob", [False, True])
@pytest.mark.parametrize("bounds", [(500, 2000), (2000, 2000)])  # KLD-adaptive and fixed-size resampling
def test_an_enabled_cycle_is_the_cycle_of_the_kept_points(prob, bounds):
    grid, truth, angles, _ = turtlebot_scene(seed=2)
    sensor = LF_PROB if prob else LF
    prm = AmclParams(min_particles=bounds[0], max_particles=bounds[1], update_min_d=0.0, update_min_a=0.0, resample_interval=2)
    a, b, c = (Amcl(grid, MOTION, sensor, prm, seed=33) for _ in range(3))
    a.set_beam_skip(True)
    for f in (a, b):
        f.initialize(truth, np.diag([0.02, 0.02, 0.01]))
    field, level = a.likelihood_field(), check_level(a, 0.5)
    pulled = np.zeros(len(angles), dtype=bool)
    pulled[40:70] = True
    pose, previous, skipped_somewhere = truth, None, 0
    for k in range(1, 7):
        pose = synth.odometry_step(pose, 0.03, 0.02)
        ranges = synth.cast_scan(grid.cells, grid.resolution, (grid.origin[2], grid.origin[3]), pose, angles, 3.5)
        points = synth.scan_points(np.where(pulled, 0.4 * ranges, ranges), angles)
        ctrl = se2_from_xytheta(*pose)
        # the set A's propagation leaves, repeated on a third context from A's set as it stands
        before = a.particles()
        c.set_particles(before[0], before[1])
        c.propagate(ctrl, ctrl if previous is None else previous, k)
        want_counts = bref.agreement_counts(field, level, grid.resolution, grid.origin, c.particles()[0], points)
        got_a = a.update(ctrl, points)
        r = a.beam_skip_result()
        assert r["valid"] and r["num_beams"] == len(points) and r["num_particles"] == len(before[0])
        assert np.array_equal(r["counts"].astype(np.int64), want_counts), k
        kept, skipped, used_all = bref.decide(want_counts, len(before[0]), len(points), a.beam_skip())
        assert np.array_equal(r["kept"], kept) and r["num_skipped"] == skipped and r["used_all"] == used_all
        skipped_somewhere += 0 if used_all else skipped
        got_b = b.update(ctrl, points if used_all else points[kept])
        assert same_bits(got_a[0], got_b[0]) and same_bits(got_a[1], got_b[1]), k
        assert a.last_info == b.last_info, k
        sa, sb = a.particles(), b.particles()
        assert same_bits(sa[0], sb[0]) and same_bits(sa[1], sb[1]), k
        previous = ctrl
    assert skipped_somewhere > 0  # (the cycles did skip)
    for f in (a, b, c):
        f.close()


def test_off_is_off():
    grid, truth, angles, ranges = turtlebot_scene()
    points = synth.scan_points(ranges, angles)
    prm = AmclParams(min_particles=500, max_particles=2000, update_min_d=0.0, update_min_a=0.0)
    toggled, never = (Amcl(grid, MOTION, LF, prm, seed=5) for _ in range(2))
    toggled.set_beam_skip(True, distance=0.4, threshold=0.2, error_threshold=0.8)
    toggled.set_beam_skip(False)
    assert toggled.beam_skip() == dict(enabled=False, distance=0.4, threshold=0.2, error_threshold=0.8)
    for f in (toggled, never):
        f.initialize(truth, np.diag([0.05, 0.05, 0.02]))
    pose = truth
    for k in range(3):
        pose = synth.odometry_step(pose, 0.05, 0.02)
        ctrl = se2_from_xytheta(*pose)
        results = [f.update(ctrl, points) for f in (toggled, never)]
        assert same_bits(results[0][0], results[1][0]) and same_bits(results[0][1], results[1][1]) and toggled.last_info == never.last_info
        a, b = snapshot(toggled), snapshot(never)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and a[2] == b[2]
        assert toggled.counter("beam_skip_launches") == 0 and not toggled.beam_skip_result()["valid"]
    for f in (toggled, never):
        f.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_other_sensor_models_and_bad_parameters_are_refused():
    lib = capi.load()
    for kind in (capi.MCL_SENSOR_BEAM, capi.MCL_SENSOR_NDT, capi.MCL_SENSOR_LANDMARK, capi.MCL_SENSOR_BEARING):
        cfg = capi.Config()
        lib.mcl_default_config(C.byref(cfg))
        cfg.sensor_kind = kind
        ctx = capi._ctx()
        assert lib.mcl_create(C.byref(cfg), C.byref(ctx)) == capi.MCL_OK
        p = capi.BeamSkipParams(1, 0, 0.5, 0.3, 0.9)
        r = capi.BeamSkipResult()
        counts = (C.c_uint32 * 2)()
        pts = (C.c_double * 4)(1.0, 0.0, 0.0, 1.0)
        U = capi.MCL_ERR_UNSUPPORTED
        assert lib.mcl_set_beam_skip(ctx, C.byref(p)) == U and lib.mcl_get_beam_skip(ctx, C.byref(p)) == U
        assert lib.mcl_get_beam_skip_result(ctx, C.byref(r), None, None, 0) == U and lib.mcl_beam_agreement(ctx, pts, 2, counts) == U
        lib.mcl_destroy(ctx)
    grid, truth, angles, ranges = turtlebot_scene()
    f = Amcl(grid, MOTION, LF, AmclParams(min_particles=100, max_particles=100), seed=1)
    f.set_beam_skip(True, distance=0.4)
    for bad in (dict(distance=0.0), dict(distance=-1.0), dict(distance=float("inf")), dict(distance=float("nan")), dict(threshold=-0.1),
                dict(threshold=1.1), dict(threshold=float("nan")), dict(error_threshold=-0.1), dict(error_threshold=2.0)):
        with pytest.raises(capi.MclError) as e:
            f.set_beam_skip(True, **bad)
        assert e.value.status == capi.MCL_ERR_INVALID_ARGUMENT
        assert f.beam_skip() == dict(enabled=True, distance=0.4, threshold=0.3, error_threshold=0.9)
    p = capi.BeamSkipParams(2, 0, 0.5, 0.3, 0.9)
    assert f._lib.mcl_set_beam_skip(f._ctx, C.byref(p)) == capi.MCL_ERR_INVALID_ARGUMENT
    # capacity below num_beams with an array given
    f.initialize(truth, np.diag([0.05, 0.05, 0.02]))
    f.reweight(synth.scan_points(ranges, angles))
    r, counts = capi.BeamSkipResult(), (C.c_uint32 * 4)()
    assert f._lib.mcl_get_beam_skip_result(f._ctx, C.byref(r), counts, None, 4) == capi.MCL_ERR_INVALID_ARGUMENT
    assert f._lib.mcl_get_beam_skip_result(f._ctx, C.byref(r), None, None, 0) == capi.MCL_OK and r.valid == 1 and r.num_beams == len(angles)
    f.close()
    # no map, no particles
    g = Amcl(grid, MOTION, LF, AmclParams(min_particles=100, max_particles=100), seed=1)
    with pytest.raises(capi.MclError) as e:
        g.beam_agreement(np.ones((3, 2)))
    assert e.value.status == capi.MCL_ERR_NOT_READY
    g.close()


class Transport(C.Structure):
    _fields_ = [("user", C.c_void_p), ("all_gather", C.c_void_p), ("all_to_all", C.c_void_p)]


GATHER = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)
EXCHANGE = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def test_several_ranks_are_refused_before_any_collective():
    grid = turtlebot()
    called = []
    gather = GATHER(lambda *a: called.append("all_gather") or -1)
    exchange = EXCHANGE(lambda *a: called.append("all_to_all") or -1)
    transport = Transport(None, C.cast(gather, C.c_void_p), C.cast(exchange, C.c_void_p))
    prm = AmclParams(min_particles=1000, max_particles=1000)
    f = Amcl(grid, MOTION, LF, prm, seed=1, shard_offset=0, shard_capacity=1000)
    f.set_beam_skip(True)
    assert f._lib.mcl_comm_attach(f._ctx, 0, 2, C.addressof(transport)) == capi.MCL_ERR_UNSUPPORTED
    assert f._lib.mcl_comm_attach_rccl(f._ctx, bytes(128), 0, 2) == capi.MCL_ERR_UNSUPPORTED
    assert not called
    assert f._lib.mcl_comm_attach(f._ctx, 0, 1, None) == capi.MCL_OK  # a world of one is allowed
    assert f.beam_skip()["enabled"]
    f.close()

    # a context attached to two ranks refuses to be enabled.  The attach's one collective compares a word of the ranks'
    # configurations: this transport answers it with the rank's own word in both places (a peer configured alike).
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]

    def echo(user, d_send, d_recv, nbytes, stream):
        called.append("echo")
        if hip.hipStreamSynchronize(stream) != 0:
            return -1
        for rank in range(2):
            if hip.hipMemcpy(d_recv + rank * nbytes, d_send, nbytes, 3) != 0:  # hipMemcpyDeviceToDevice
                return -1
        return 0
    gather2 = GATHER(echo)
    transport2 = Transport(None, C.cast(gather2, C.c_void_p), C.cast(exchange, C.c_void_p))
    g = Amcl(grid, MOTION, LF, prm, seed=1, shard_offset=0, shard_capacity=1000)
    assert g._lib.mcl_comm_attach(g._ctx, 0, 2, C.addressof(transport2)) == capi.MCL_OK
    seen = list(called)
    with pytest.raises(capi.MclError) as e:
        g.set_beam_skip(True)
    assert e.value.status == capi.MCL_ERR_UNSUPPORTED and called == seen and not g.beam_skip()["enabled"]
    g.set_beam_skip(False, distance=0.4)  # (the parameters may change while it stays off)
    g.close()


# ---- 6. a batch --------------------------------------------------------------------------------------------------------------------------------
def test_a_batch_member_with_skipping_on_runs_its_lone_cycle():
    grid, truth, angles, _ = turtlebot_scene()
    sizes = (500, 1000, 1500, 2000)
    skipping = (1, 3)
    specs = [dict(grid=grid, motion=MOTION, sensor=LF, params=AmclParams(min_particles=n, max_particles=n, update_min_d=0.0, update_min_a=0.0), seed=40 + i)
             for i, n in enumerate(sizes)]
    fleet = AmclBatch(specs)
    lone = [Amcl(s["grid"], s["motion"], s["sensor"], s["params"], seed=s["seed"]) for s in specs]
    for i in skipping:
        fleet.members[i].set_beam_skip(True)
        lone[i].set_beam_skip(True)
    for f in list(fleet.members) + lone:
        f.initialize(truth, np.diag([0.02, 0.02, 0.01]))
    pulled = np.zeros(len(angles), dtype=bool)
    pulled[40:70] = True
    pose = truth
    for k in range(3):
        pose = synth.odometry_step(pose, 0.03, 0.02)
        ranges = synth.cast_scan(grid.cells, grid.resolution, (grid.origin[2], grid.origin[3]), pose, angles, 3.5)
        points = synth.scan_points(np.where(pulled, 0.4 * ranges, ranges), angles)
        ctrl = se2_from_xytheta(*pose)
        alone, fused = fleet.counter("members_alone"), fleet.counter("members_fused")
        got = fleet.update([ctrl] * 4, [points] * 4)
        assert fleet.counter("members_alone") == alone + 2 and fleet.counter("members_fused") == fused + 2
        for i, f in enumerate(lone):
            want = f.update(ctrl, points)
            assert same_bits(got[i][0], want[0]) and same_bits(got[i][1], want[1]), (k, i)
            assert fleet.last_infos[i] == f.last_info
            sa, sb = fleet.members[i].particles(), f.particles()
            assert same_bits(sa[0], sb[0]) and same_bits(sa[1], sb[1])
            if i in skipping:
                ra, rb = fleet.members[i].beam_skip_result(), f.beam_skip_result()
                assert ra["valid"] and np.array_equal(ra["counts"], rb["counts"]) and np.array_equal(ra["kept"], rb["kept"])
    assert any(lone[i].beam_skip_result()["num_skipped"] > 0 for i in skipping)
    for f in lone:
        f.close()
    fleet.close()
