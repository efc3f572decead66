"""mcl_batch_*: a fleet of small filters behind one update call (DESIGN.md "Batched small filters").

The yardstick is always a TWIN: a lone Amcl with the same config, seed and map, initialised the same way and driven by mcl_update with
the same inputs.  Every comparison is np.array_equal - estimate, every field of mcl_update_info, the particle states and weights after
every cycle, the particle count.  The twin is the path test_gpu_parity.py holds to the oracle."""
import numpy as np
import pytest

from beluga_amd import capi, synth
from beluga_amd.amcl import (Amcl, AmclBatch, AmclParams, BeamModelParam, LikelihoodFieldProbModelParam, OccupancyGrid,
                             OmnidirectionalDriveModelParam, StationaryModelParam, se2_from_xytheta)
from test_gpu_parity import LF, MOTION, rooms_grid

pytestmark = pytest.mark.gpu

COV = np.diag([0.04, 0.04, 0.01])
LF_PROB = LikelihoodFieldProbModelParam(2.0, 100.0, 0.5, 0.5, 0.2, True)
OMNI = OmnidirectionalDriveModelParam(0.1, 0.05, 0.1, 0.05, 0.02)
BEAM = BeamModelParam(beam_max_range=12.0)


def wide_grid():
    """128 x 64 cells: another height than the square maps, so that the shared reweight's workgroup memory is a maximum over members."""
    cells = synth.make_rooms_map(128, 64, seed=9, n_rooms=3)
    return OccupancyGrid(cells=cells, resolution=0.05, origin=se2_from_xytheta(-3.2, -1.6, 0.0))


class World:
    """A map, a robot driving through it, and the scans it sees (cached per cycle and beam count: a reference computed once)."""

    def __init__(self, grid, seed=3):
        self.grid = grid
        self.origin_xy = (grid.origin[2], grid.origin[3])
        self.start = synth.find_free_pose(grid.cells, grid.resolution, self.origin_xy, seed=seed, clearance_cells=5)
        self._scans = {}

    def pose(self, cycle):
        p = self.start
        for _ in range(cycle):
            p = synth.odometry_step(p, 0.3, 0.9)  # (turning: the robot stays inside a small map)
        return p

    def odom(self, cycle):
        p = (0.0, 0.0, 0.0)
        for _ in range(cycle):
            p = synth.odometry_step(p, 0.3, 0.9)
        return se2_from_xytheta(*p)

    def scan(self, cycle, beams):
        if beams == 0:
            return np.zeros((0, 2))
        key = (cycle, beams)
        if key not in self._scans:
            angles = synth.lidar_angles(beams, 270.0)
            ranges = synth.cast_scan(self.grid.cells, self.grid.resolution, self.origin_xy, self.pose(cycle), angles, 8.0, 0.01, seed=cycle)
            self._scans[key] = synth.scan_points(ranges, angles)
        return self._scans[key]


@pytest.fixture(scope="module")
def worlds():
    return {"a": World(rooms_grid(96, 3)), "b": World(wide_grid())}


def spec(world, lo, hi, seed, beams, sensor=LF, motion=MOTION, options=None, **params):
    return dict(world=world, params=AmclParams(min_particles=lo, max_particles=hi, **params), seed=seed, beams=beams, sensor=sensor,
                motion=motion, options=options)


class Fleet:
    """A batch and, member by member, its twins."""

    def __init__(self, worlds, specs, with_map=None):
        self.specs = specs
        self.worlds = [worlds[s["world"]] for s in specs]
        with_map = with_map or [True] * len(specs)
        args = [dict(grid=w.grid if has else None, motion=s["motion"], sensor=s["sensor"], params=s["params"], seed=s["seed"],
                     options=s["options"]) for s, w, has in zip(specs, self.worlds, with_map)]
        self.batch = AmclBatch(args)
        self.twins = [Amcl(w.grid, s["motion"], s["sensor"], s["params"], seed=s["seed"], options=s["options"]) if has else None
                      for s, w, has in zip(specs, self.worlds, with_map)]
        for i, (w, has) in enumerate(zip(self.worlds, with_map)):
            if has:
                self.both(i, lambda f, w=w: f.initialize(w.start, COV))
        self.cycle = 0
        self.controls = [w.odom(0) for w in self.worlds]

    def both(self, i, call):
        call(self.batch.members[i])
        call(self.twins[i])

    def inputs(self, hold=()):
        """This cycle's control action and scan per member; a member in `hold` gets the control it had last (no motion)."""
        c = self.cycle + 1
        controls = [self.controls[i] if i in hold else w.odom(c) for i, w in enumerate(self.worlds)]
        scans = [w.scan(c, s["beams"]) for w, s in zip(self.worlds, self.specs)]
        return controls, scans

    def step(self, hold=(), skip_twins=(), check=True):
        """One batch update and the same update on every twin; everything compared."""
        controls, scans = self.inputs(hold)
        got = self.batch.update(controls, scans, check=check)
        self.controls = controls
        infos = self.batch.last_infos
        for i, twin in enumerate(self.twins):
            if twin is None or i in skip_twins:
                continue
            want = twin.update(controls[i], scans[i])
            self.compare(i, got[i], want, infos[i])
        self.cycle += 1
        return got

    def compare(self, i, got, want, info=None):
        member, twin = self.batch.members[i], self.twins[i]
        at = f"member {i}, cycle {self.cycle}"
        assert (got is None) == (want is None), at
        if want is not None:
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), at
        if info is not None:
            assert info.keys() == twin.last_info.keys()
            for key, value in twin.last_info.items():
                assert np.array_equal(np.float64(info[key]), np.float64(value), equal_nan=True), f"{at}: {key} {info[key]} != {value}"
        assert member.num_particles() == twin.num_particles(), at
        gs, gw = member.particles()
        ws, ww = twin.particles()
        assert np.array_equal(gs, ws), at
        assert np.array_equal(gw, ww), at

    def close(self):
        self.batch.close()
        for twin in self.twins:
            if twin is not None:
                twin.close()


def test_mixed_fleet(worlds):
    """Six members that differ in everything: the edges of the 256-particle block, of the 4-particle reweight block and of the 4096 cap;
    scans with and without a four-per-lane part, and an empty one; two maps of different height; the prob model; all three motion
    models; KLD-adaptive and fixed sizes."""
    fleet = Fleet(worlds, [
        spec("a", 257, 257, 11, 61),
        spec("b", 301, 301, 12, 180, sensor=LF_PROB),
        spec("a", 2000, 2000, 13, 259, motion=OMNI),
        spec("b", 500, 2000, 14, 1080),
        spec("a", 4096, 4096, 15, 0),
        spec("b", 64, 300, 16, 180, motion=StationaryModelParam()),
    ])
    for _ in range(6):
        out = fleet.step()
        assert all(o is not None for o in out)
    assert fleet.batch.counter("members_fused") == 36 and fleet.batch.counter("members_alone") == 0
    assert fleet.batch.counter("cycles") == 6 and fleet.batch.counter("kernel_launches") == 18
    fleet.close()


def test_policies(worlds):
    """selective_resampling, resample_interval = 2, a member that stands still in cycles 2 and 3, and a member with injected random
    states, which come from its OWN map's free cells."""
    fleet = Fleet(worlds, [
        spec("a", 500, 500, 21, 180, selective_resampling=True),
        spec("b", 500, 500, 22, 180, resample_interval=2),
        spec("a", 300, 1000, 23, 61),
        spec("b", 700, 700, 24, 180),
    ])
    fleet.both(3, lambda f: f.debug_set_recovery_filters(1.0, 0.5))
    injected = False
    for c in range(5):
        still = (2,) if c in (2, 3) else ()
        before = fleet.batch.members[2].particles() if still else None
        out = fleet.step(hold=still)
        injected = injected or fleet.batch.last_infos[3]["random_state_probability"] > 0.0
        if still:  # updated = 0: the member's state is as it was, the others advanced
            assert out[2] is None and not fleet.batch.last_infos[2]["updated"]
            after = fleet.batch.members[2].particles()
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
            assert all(out[i] is not None for i in (0, 1, 3))
    assert injected  # (the twin draws them from map b's free cells, and the member equals it)
    fleet.close()


def test_cluster_based_estimate_member(worlds):
    fleet = Fleet(worlds, [spec("a", 600, 600, 31, 180), spec("b", 400, 1200, 32, 180)])
    fleet.both(0, lambda f: f.set_estimate_kind(cluster_based=True))
    for _ in range(3):
        fleet.step()
    assert fleet.batch.counter("members_fused") == 6
    fleet.close()


def test_members_that_do_not_qualify_run_beside_fused_ones(worlds):
    fleet = Fleet(worlds, [
        spec("a", 1000, 1000, 41, 180),
        spec("b", 5000, 5000, 42, 180),                           # beyond 4096 particles
        spec("a", 300, 300, 43, 61, sensor=BEAM),                 # the beam model
        spec("b", 800, 800, 44, 180, options={"small_fused": 0}),  # the kernels of the large path
        spec("b", 200, 900, 45, 259),
    ])
    for _ in range(3):
        fleet.step()
    assert fleet.batch.counter("members_fused") == 6 and fleet.batch.counter("members_alone") == 9
    assert fleet.batch.counter("kernel_launches") == 9 and fleet.batch.counter("cycles") == 3
    fleet.close()


def test_it_is_really_batched(worlds):
    """The launches of a cycle do not depend on the number of members (without this, a loop over mcl_update would pass everything else)."""
    per_cycle = []
    for members in (2, 9):
        fleet = Fleet(worlds, [spec("ab"[i % 2], 300 + 50 * i, 300 + 50 * i, 50 + i, 180) for i in range(members)])
        tails = [m.counter("small_tail_launches") for m in fleet.batch.members]
        for c in range(3):
            before = fleet.batch.counter("kernel_launches")
            fleet.step()
            per_cycle.append(fleet.batch.counter("kernel_launches") - before)
            assert [m.counter("small_tail_launches") for m in fleet.batch.members] == [t + c + 1 for t in tails]
        assert fleet.batch.counter("members_fused") == 3 * members
        fleet.close()
    assert len(set(per_cycle)) == 1 and 1 <= per_cycle[0] <= 3, per_cycle


@pytest.mark.parametrize("members", [1, 33])
def test_edges_of_the_member_search(worlds, members):
    """One member, and 33 members of one propagation block and 16 reweight blocks each (a prefix that is no power of two)."""
    if members == 1:
        fleet = Fleet(worlds, [spec("a", 777, 777, 61, 180)])
    else:
        fleet = Fleet(worlds, [spec("ab"[i % 2], 64, 64, 100 + i, 16) for i in range(33)])
    for _ in range(2):
        fleet.step()
    assert fleet.batch.counter("members_fused") == 2 * members
    fleet.close()


def test_state_lives_in_the_members(worlds):
    fleet = Fleet(worlds, [spec("a", 400, 400, 71, 180), spec("b", 300, 900, 72, 61), spec("a", 500, 500, 73, 259)])
    for _ in range(2):
        fleet.step()
    # mcl_update on member 1 directly: its control moves on, the others' does not (the batch sees them one cycle behind)
    w = fleet.worlds[1]
    control, scan = w.odom(fleet.cycle + 1), w.scan(fleet.cycle + 1, 61)
    got = fleet.batch.members[1].update(control, scan)
    want = fleet.twins[1].update(control, scan)
    fleet.compare(1, got, want)
    states = synth.normal_particles(450, fleet.worlds[2].pose(fleet.cycle), (0.2, 0.2, 0.1), seed=5)
    weights = np.linspace(0.5, 1.5, 450)
    fleet.both(2, lambda f: f.set_particles(states, weights))
    fleet.cycle += 1  # (member 1 has seen this cycle's control already; cycle + 2 moves everyone)
    for _ in range(2):
        fleet.step()
    fleet.close()


def test_errors(worlds):
    fleet = Fleet(worlds, [spec("a", 300, 300, 81, 61), spec("b", 300, 300, 82, 61), spec("a", 300, 300, 83, 61)], with_map=[True, False, True])
    lost = synth.normal_particles(300, (0.0, 0.0, 0.0), (0.2, 0.2, 0.1), seed=8)  # (particles, but no map to weigh them on)
    fleet.batch.members[1].set_particles(lost, np.ones(300))
    out = fleet.step(check=False)  # the member without a map fails as its own mcl_update does; the others advance (compared in step)
    assert fleet.batch.last_status == capi.MCL_ERR_NOT_READY
    assert fleet.batch.statuses == [capi.MCL_OK, capi.MCL_ERR_NOT_READY, capi.MCL_OK]
    assert out[0] is not None and out[1] is None and out[2] is not None
    states, weights = fleet.batch.members[1].particles()  # as its own failing mcl_update leaves it: untouched
    assert np.array_equal(states, lost) and np.array_equal(weights, np.ones(300))
    # offsets that decrease: refused, and no member moves
    before = [fleet.batch.members[i].particles() for i in (0, 2)]
    controls, _ = fleet.inputs()
    status = fleet.batch.update_offsets(controls, np.zeros((8, 2)), [0, 8, 4, 8])
    assert status == capi.MCL_ERR_INVALID_ARGUMENT
    for (s0, w0), i in zip(before, (0, 2)):
        s1, w1 = fleet.batch.members[i].particles()
        assert np.array_equal(s0, s1) and np.array_equal(w0, w1)
    # mcl_destroy on a member leaves the batch usable
    lib = capi.load()
    lib.mcl_destroy(fleet.batch.members[0]._ctx)
    fleet.batch.members[0].close()
    fleet.step(check=False)
    assert fleet.batch.statuses[0] == capi.MCL_OK and fleet.batch.statuses[2] == capi.MCL_OK
    fleet.close()
    # two device ids, mixed streams
    a = dict(grid=None, motion=MOTION, sensor=LF, params=AmclParams(min_particles=100, max_particles=100))
    for other in (dict(a, device=1), dict(a, hip_stream=0x1000)):
        with pytest.raises(capi.MclError) as e:
            AmclBatch([a, other])
        assert e.value.status == capi.MCL_ERR_INVALID_ARGUMENT
