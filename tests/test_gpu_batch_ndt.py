"""NDT members of a fleet on the shared launches (mcl_batch_update with the members' switch mcl_set_ndt_small_cycle; DESIGN.md "Batched
small filters").

The yardstick is test_gpu_batch.py's: a TWIN per member - a lone Amcl with the same config, switch, seed and map, initialised the same
way and driven by mcl_update with the same inputs.  Every comparison is np.array_equal: estimate and covariance, every field of
mcl_update_info, the status, the particle count, the states and weights after every cycle."""
import numpy as np
import pytest

from beluga_amd import capi, synth
from beluga_amd.amcl import Amcl, AmclBatch, AmclParams, se2_from_xytheta
from test_gpu_batch import COV, MOTION, World, spec
from test_gpu_batch_beam import BeamFleet, beam
from test_gpu_ndt import NODE, ring_scan, turtlebot_ndt
from test_gpu_ndt_small import collapsed, patchwork_ndt
from test_gpu_parity import rooms_grid

pytestmark = pytest.mark.gpu


class NdtWorld:
    """An NDT map, a robot that drives a slow arc through it, and the scans it sees."""

    def __init__(self, ndt_map, start):
        self.grid = ndt_map
        self.start = start

    def odom(self, cycle):
        p = (0.0, 0.0, 0.0)
        for _ in range(cycle):
            p = synth.odometry_step(p, 0.3, 0.05)
        return se2_from_xytheta(*p)

    def scan(self, cycle, beams):
        """beams < 5: no cell of five points, so no measurement cell at all (K = 0)."""
        return ring_scan((0.0, 0.0), beams, seed=cycle) if beams else np.zeros((0, 2))


@pytest.fixture(scope="module")
def worlds():
    return {"t": NdtWorld(turtlebot_ndt(), (-0.5, 0.3, 0.2)), "p": NdtWorld(patchwork_ndt(), (-1.0, -0.5, 0.4)),
            "a": World(rooms_grid(96, 3))}


def ndt(world, lo, hi, seed, beams, small=True, **params):
    return dict(spec(world, lo, hi, seed, beams, sensor=NODE, **params), small=small)


class NdtFleet(BeamFleet):
    """BeamFleet (its comparison holds NaNs to the twin's: the covariance of one particle) whose members may carry the NDT switch."""

    def __init__(self, worlds, specs):
        self.specs = specs
        self.worlds = [worlds[s["world"]] for s in specs]

        def more(s):
            return dict(seed=s["seed"], options=s["options"], **({"ndt_small_cycle": True} if s.get("small") else {}))

        self.batch = AmclBatch([dict(grid=w.grid, motion=s["motion"], sensor=s["sensor"], params=s["params"], **more(s))
                                for s, w in zip(specs, self.worlds)])
        self.twins = [Amcl(w.grid, s["motion"], s["sensor"], s["params"], **more(s)) for s, w in zip(specs, self.worlds)]
        for i, w in enumerate(self.worlds):
            self.both(i, lambda f, w=w: f.initialize(w.start, COV))
        self.cycle = 0
        self.controls = [w.odom(0) for w in self.worlds]

    def small_counts(self, i):
        got, want = self.batch.members[i].ndt_small_cycle_counts(), self.twins[i].ndt_small_cycle_counts()
        assert got == want, f"member {i}, cycle {self.cycle}"
        return got


def counters(fleet):
    out = {k: fleet.batch.counter(k) for k in ("cycles", "kernel_launches", "members_fused", "members_alone", "beam_launches",
                                                "members_beam_fused", "cluster_launches", "members_cluster_fused")}
    out["ndt_launches"], out["members_ndt_fused"] = fleet.batch.ndt_counts()
    return out


def test_shapes_at_the_kernels_edges(worlds):
    """The four-particle block and its tail (1, 4, 5), more than one propagation block (500), a KLD-adaptive member (500 .. 2000), the
    cap (4096); two maps, scans of different sizes and one without a measurement cell, whose weights stay untouched; one member with
    the switch off, which runs its own cycle."""
    fleet = NdtFleet(worlds, [
        ndt("t", 1, 1, 211, 360),
        ndt("p", 4, 4, 212, 720),
        ndt("t", 5, 5, 213, 4),
        ndt("t", 500, 2000, 214, 360),
        ndt("p", 4096, 4096, 215, 180),
        ndt("t", 2000, 2000, 216, 360, small=False),
        ndt("p", 500, 500, 217, 1080, resample_interval=2),
    ])
    assert [m.ndt_small_cycle() for m in fleet.batch.members] == [True, True, True, True, True, False, True]
    cycles = 4
    for _ in range(cycles):
        out = fleet.step()
        assert all(o is not None for o in out)
    got = counters(fleet)
    assert got["members_ndt_fused"] == 6 * cycles and got["members_fused"] == 6 * cycles and got["members_alone"] == cycles, got
    assert got["kernel_launches"] == 3 * cycles and got["ndt_launches"] == cycles and got["cycles"] == cycles, got
    assert got["beam_launches"] == 0
    for i in (0, 1, 2, 3, 4, 6):
        assert sum(fleet.small_counts(i)) == cycles
    assert fleet.small_counts(5) == (0, 0)
    fleet.close()


def test_mixed_families(worlds):
    """A likelihood-field member, a fused beam member and NDT members in one fleet: a reweight launch per family between the shared
    propagation and the shared tail - five launches; three for a fleet of NDT members alone."""
    fleet = NdtFleet(worlds, [
        spec("a", 300, 300, 221, 180),
        ndt("t", 301, 301, 222, 360),
        beam("a", 257, 257, 223, 61),
        ndt("p", 64, 300, 224, 720),
    ])
    for c in range(3):
        before = counters(fleet)
        fleet.step()
        after = counters(fleet)
        assert after["kernel_launches"] - before["kernel_launches"] == 5, (c, before, after)
        assert after["beam_launches"] - before["beam_launches"] == 1 and after["ndt_launches"] - before["ndt_launches"] == 1, (c, before, after)
    got = counters(fleet)
    assert got["members_fused"] == 12 and got["members_beam_fused"] == 3 and got["members_ndt_fused"] == 6 and got["members_alone"] == 0, got
    fleet.close()
    alone = NdtFleet(worlds, [ndt("t", 300, 300, 225, 360), ndt("p", 257, 257, 226, 61)])
    for c in range(2):
        before = alone.batch.counter("kernel_launches")
        alone.step()
        assert alone.batch.counter("kernel_launches") - before == 3
    alone.close()


def test_hand_back_and_a_refused_generator_stay_the_members_own(worlds):
    """Three NDT members: one whose filters never move apart (every cycle ends in the tail), one whose filters are put apart (its first
    cycle is handed back and finished inside the call) and one whose set is collapsed as well (its generator is refused).  The failing
    member's status and state are its lone mcl_update's; the others' results are their twins', untouched."""
    fleet = NdtFleet(worlds, [
        ndt("t", 300, 300, 231, 360, alpha_slow=0.05, alpha_fast=0.05),
        ndt("t", 301, 301, 232, 360),
        ndt("p", 64, 64, 233, 4),  # (four points: no measurement cell - the weights stay equal and the collapsed set's headings cancel)
        ndt("p", 257, 257, 234, 61, alpha_slow=0.05, alpha_fast=0.05),
    ])
    fleet.both(1, lambda f: f.debug_set_recovery_filters(2.0 / 301, 0.5 / 301))
    fleet.both(2, lambda f: f.set_particles(collapsed(64), np.ones(64)))
    fleet.both(2, lambda f: f.debug_set_recovery_filters(2.0 / 64, 0.5 / 64))
    controls, scans = fleet.inputs()
    with pytest.raises(capi.MclError) as lone:
        fleet.twins[2].update(controls[2], scans[2])
    assert lone.value.status == capi.MCL_ERR_BAD_COVARIANCE
    out = fleet.step(skip_twins=(2,), check=False)
    assert fleet.batch.statuses == [capi.MCL_OK, capi.MCL_OK, capi.MCL_ERR_BAD_COVARIANCE, capi.MCL_OK]
    assert fleet.batch.last_status == capi.MCL_ERR_BAD_COVARIANCE
    assert out[2] is None and all(out[i] is not None for i in (0, 1, 3))
    gs, gw = fleet.batch.members[2].particles()
    ws, ww = fleet.twins[2].particles()
    assert np.array_equal(gs, ws) and np.array_equal(gw, ww) and len(gs) == 64 and np.all(gw == 1.0 / 64)
    assert fleet.small_counts(0) == (1, 0) and fleet.small_counts(3) == (1, 0)
    assert fleet.small_counts(1) == (0, 1) and fleet.small_counts(2) == (0, 1)  # handed back, both; one finished inside the call
    # the next cycle: the control has moved, the propagation's noise takes the failed member's set apart and its generator stands
    # (its filters were advanced, not reset: handed back again); the reset filters of member 1 keep its cycle in the tail
    out = fleet.step()
    assert all(o is not None for o in out) and fleet.batch.statuses == [capi.MCL_OK] * 4
    assert fleet.small_counts(0) == (2, 0) and fleet.small_counts(3) == (2, 0)
    assert fleet.small_counts(1) == (1, 1) and fleet.small_counts(2) == (0, 2)
    got = counters(fleet)
    assert got["members_fused"] == 7 and got["members_ndt_fused"] == 7 and got["members_alone"] == 0 and got["kernel_launches"] == 6, got
    fleet.close()


def test_cluster_based_estimate_of_a_fused_ndt_member(worlds):
    fleet = NdtFleet(worlds, [ndt("t", 600, 600, 241, 360), ndt("p", 400, 1200, 242, 720, alpha_slow=0.05, alpha_fast=0.05)])
    fleet.both(0, lambda f: f.set_estimate_kind(cluster_based=True))
    fleet.both(1, lambda f: f.set_estimate_kind(cluster_based=True))
    fleet.both(0, lambda f: f.debug_set_recovery_filters(2.0 / 600, 0.5 / 600))  # its first cycle is handed back: its own estimate
    for _ in range(3):
        fleet.step()
    got = counters(fleet)
    done, back = fleet.small_counts(0)
    assert back >= 1 and done + back == 3 and fleet.small_counts(1) == (3, 0)
    assert got["members_ndt_fused"] == 6 and got["members_cluster_fused"] == 3 + done and got["cluster_launches"] > 0, got
    fleet.close()
