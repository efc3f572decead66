"""Beam-model members of a fleet on the shared launches (mcl_batch_update with the members' option batch_beam_fused; DESIGN.md "Batched
small filters").

The yardstick is test_gpu_batch.py's: a TWIN per member - a lone Amcl with the same config, options, seed and map, initialised the same
way and driven by mcl_update with the same inputs.  Every comparison is np.array_equal: estimate and covariance, every field of
mcl_update_info, the particle count, the states and weights after every cycle - and, for a beam member, the cells its ray walks visited
(mcl_beam_cells_visited), which the shared kernel adds to the member's own word."""
import numpy as np
import pytest

from beluga_amd import capi
from beluga_amd.amcl import BeamModelParam, StationaryModelParam
from test_gpu_batch import LF_PROB, OMNI, Fleet, World, spec, wide_grid
from test_gpu_parity import LF, rooms_grid

pytestmark = pytest.mark.gpu

BEAM = BeamModelParam(beam_max_range=12.0)
ON = {"batch_beam_fused": 1}


@pytest.fixture(scope="module")
def worlds():
    return {"a": World(rooms_grid(96, 3)), "b": World(wide_grid())}


def beam(world, lo, hi, seed, beams, options=ON, **more):
    return spec(world, lo, hi, seed, beams, sensor=BEAM, options=options, **more)


class BeamFleet(Fleet):
    """Fleet whose comparison also holds NaNs to the twin's (the covariance of a single particle) and a beam member's visited cells."""

    def compare(self, i, got, want, info=None):
        at = f"member {i}, cycle {self.cycle}"
        assert (got is None) == (want is None), at
        if want is not None:
            assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1], equal_nan=True), at
            finite = np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
            super().compare(i, got if finite else None, want if finite else None, info)
        else:
            super().compare(i, got, want, info)
        if self.specs[i]["sensor"] is BEAM:
            assert self.batch.members[i].beam_cells_visited(reset=False) == self.twins[i].beam_cells_visited(reset=False), at


def counters(fleet):
    return {k: fleet.batch.counter(k) for k in ("cycles", "kernel_launches", "members_fused", "members_alone", "beam_launches",
                                                "members_beam_fused", "cluster_launches", "members_cluster_fused")}


def test_shapes_at_the_kernels_edges(worlds):
    """The 4-particle block and its tail (1, 4, 5), the propagation block's edge (257), the cap (4096); the lane loop's edge (63, 64,
    65), one point, the workgroup memory's limit (4096 points) and an empty scan, whose weights stay untouched; two maps of different
    size; all three motion models; a KLD-adaptive member; resample_interval = 2."""
    fleet = BeamFleet(worlds, [
        beam("a", 1, 1, 111, 63),
        beam("b", 4, 4, 112, 64, motion=OMNI),
        beam("a", 5, 5, 113, 4096),
        beam("b", 257, 257, 114, 65, motion=StationaryModelParam()),
        beam("a", 4096, 4096, 115, 1),
        beam("b", 300, 300, 116, 0),
        beam("a", 64, 300, 117, 180),
        beam("b", 500, 500, 118, 180, resample_interval=2),
    ])
    cycles = 4
    for _ in range(cycles):
        out = fleet.step()
        assert all(o is not None for o in out)
    got = counters(fleet)
    assert got["members_beam_fused"] == 8 * cycles and got["members_fused"] == 8 * cycles and got["members_alone"] == 0, got
    assert got["kernel_launches"] == 3 * cycles and got["beam_launches"] == cycles and got["cycles"] == cycles, got
    assert fleet.batch.members[6].beam_cells_visited(reset=False) > 0
    assert fleet.batch.members[5].beam_cells_visited(reset=False) == 0  # (the empty scan: no walk)
    fleet.close()


def test_mixed_families(worlds):
    """Likelihood-field, likelihood-field-prob and beam members in one fleet: a reweight launch per family, between the shared
    propagation and the shared tail."""
    fleet = BeamFleet(worlds, [
        spec("a", 300, 300, 121, 180),
        beam("b", 301, 301, 122, 180),
        spec("b", 257, 257, 123, 61, sensor=LF_PROB),
        beam("a", 5, 5, 124, 65),
        spec("a", 64, 300, 125, 259, sensor=LF, motion=OMNI),
        beam("b", 700, 700, 126, 61),
    ])
    for c in range(3):
        before = counters(fleet)
        fleet.step()
        after = counters(fleet)
        assert after["kernel_launches"] - before["kernel_launches"] == 4, (c, before, after)
        assert after["beam_launches"] - before["beam_launches"] == 1, (c, before, after)
    got = counters(fleet)
    assert got["members_fused"] == 18 and got["members_beam_fused"] == 9 and got["members_alone"] == 0, got
    fleet.close()


def test_it_is_really_batched(worlds):
    """The launches of a cycle do not depend on the number of beam members (a loop over mcl_update would pass everything else)."""
    per_cycle = []
    for members in (2, 9):
        fleet = BeamFleet(worlds, [beam("ab"[i % 2], 100 + 30 * i, 100 + 30 * i, 150 + i, 61) for i in range(members)])
        tails = [m.counter("small_tail_launches") for m in fleet.batch.members]
        for c in range(3):
            before = fleet.batch.counter("kernel_launches")
            fleet.step()
            per_cycle.append(fleet.batch.counter("kernel_launches") - before)
            assert [m.counter("small_tail_launches") for m in fleet.batch.members] == [t + c + 1 for t in tails]
        assert fleet.batch.counter("members_beam_fused") == 3 * members and fleet.batch.counter("members_alone") == 0
        fleet.close()
    assert len(set(per_cycle)) == 1 and 1 <= per_cycle[0] <= 3, per_cycle


def test_members_that_leave_the_path(worlds):
    """Beside two fused beam members: one with the option at its default and one that wants the ordered kernel run alone, and one whose
    scan is beyond the wave-per-particle kernel's workgroup memory fails as its lone mcl_update does, untouched, while the others proceed."""
    fleet = BeamFleet(worlds, [
        beam("a", 300, 300, 131, 61),
        beam("b", 300, 300, 132, 61, options=None),                                              # the option's default: off
        beam("a", 600, 600, 133, 61, options={"batch_beam_fused": 1, "beam_sort_min_particles": 256}),  # the ordered kernel
        beam("b", 200, 200, 134, 4097),                                                          # 4097 points: refused
        beam("b", 257, 257, 135, 180),
    ])
    refused, twin = fleet.batch.members[3], fleet.twins[3]
    start = refused.particles()
    cycles = 3
    for _ in range(cycles):
        controls, scans = fleet.inputs()
        with pytest.raises(capi.MclError) as lone:
            twin.update(controls[3], scans[3])
        out = fleet.step(skip_twins=(3,), check=False)
        assert fleet.batch.statuses[3] == lone.value.status != capi.MCL_OK
        assert fleet.batch.statuses[:3] + fleet.batch.statuses[4:] == [capi.MCL_OK] * 4 and fleet.batch.last_status == lone.value.status
        assert out[3] is None and all(out[i] is not None for i in (0, 1, 2, 4))
        for filt in (refused, twin):  # as the failing mcl_update leaves it
            states, weights = filt.particles()
            assert np.array_equal(states, start[0]) and np.array_equal(weights, start[1])
    got = counters(fleet)
    assert got["members_beam_fused"] == 2 * cycles and got["members_fused"] == 2 * cycles and got["members_alone"] == 2 * cycles, got
    assert got["kernel_launches"] == 3 * cycles and got["beam_launches"] == cycles, got
    fleet.close()


def test_cluster_based_estimate_of_a_fused_beam_member(worlds):
    fleet = BeamFleet(worlds, [beam("a", 600, 600, 141, 180), beam("b", 400, 1200, 142, 61)])
    fleet.both(0, lambda f: f.set_estimate_kind(cluster_based=True))
    for _ in range(3):
        fleet.step()
    got = counters(fleet)
    assert got["members_beam_fused"] == 6 and got["members_cluster_fused"] == 3 and got["cluster_launches"] > 0, got
    fleet.close()


def test_the_option(worlds):
    """Accepted by mcl_set_option, and what it was set to last decides the member's next cycle (the library has no call that reads an
    option back: its effect on the batch's counters is what can be read)."""
    fleet = BeamFleet(worlds, [beam("a", 300, 300, 151, 61, options=None), beam("b", 257, 257, 152, 61, options=None)])
    lib = capi.load()
    assert lib.mcl_set_option(fleet.batch.members[0]._ctx, b"batch_beam_fused", 1) == capi.MCL_OK
    assert lib.mcl_set_option(None, b"batch_beam_fused", 1) == capi.MCL_ERR_INVALID_ARGUMENT
    fleet.step()
    got = counters(fleet)
    assert (got["members_beam_fused"], got["members_fused"], got["members_alone"], got["beam_launches"]) == (1, 1, 1, 1), got
    fleet.batch.set_option("batch_beam_fused", 1)
    fleet.step()
    got = counters(fleet)
    assert (got["members_beam_fused"], got["members_fused"], got["members_alone"], got["beam_launches"]) == (3, 3, 1, 2), got
    fleet.batch.set_option("batch_beam_fused", 0)
    fleet.step()
    got = counters(fleet)
    assert (got["members_beam_fused"], got["members_fused"], got["members_alone"], got["beam_launches"]) == (3, 3, 3, 2), got
    fleet.close()
