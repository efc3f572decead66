"""mcl_batch_update with members that return the cluster-based estimate (DESIGN.md "Batched small filters"): two shared launches for the
fleet in place of two launches and two synchronisations per member.

The yardstick is the one of test_gpu_batch.py: every member has a lone TWIN driven by mcl_update, and after every cycle the estimate,
every field of mcl_update_info, the particle states, the weights and the count are compared with np.array_equal."""
import numpy as np
import pytest

from beluga_amd import capi, synth
from beluga_amd.amcl import OccupancyGrid, StationaryModelParam, se2_from_xytheta
from test_gpu_batch import BEAM, COV, LF_PROB, OMNI, Fleet, World, spec, wide_grid
from test_gpu_parity import rooms_grid

pytestmark = pytest.mark.gpu


def utm_grid():
    """The square map with its origin at UTM scale: the estimate sums of a cluster there are taken about a pivot that matters."""
    cells = synth.make_rooms_map(96, 96, seed=3, n_rooms=12)
    return OccupancyGrid(cells=cells, resolution=0.05, origin=se2_from_xytheta(5.0e5, 4.0e6, 0.0))


@pytest.fixture(scope="module")
def worlds():
    return {"a": World(rooms_grid(96, 3)), "b": World(wide_grid()), "utm": World(utm_grid())}


def cluster_fleet(worlds, specs, kind0=()):
    fleet = Fleet(worlds, specs)
    for i in range(len(specs)):
        if i not in kind0:
            fleet.both(i, lambda f: f.set_estimate_kind(cluster_based=True))
    return fleet


def two_blobs(centre, apart=3.0, seed=5):
    """300 particles about `centre` and 200 about a point `apart` metres further along x, unit weights."""
    x, y, t = centre
    a = synth.normal_particles(300, (x, y, t), (0.1, 0.1, 0.05), seed=seed)
    b = synth.normal_particles(200, (x + apart, y, t), (0.1, 0.1, 0.05), seed=seed + 1)
    return np.concatenate([a, b]), np.ones(500)


def test_mixed_fleet_all_cluster_based(worlds):
    """The edges of the sizes (64, 257, the 4096 cap with an empty scan), KLD-adaptive, the prob model, the omnidirectional motion model,
    both maps, and one member of the other estimate kind between them."""
    specs = [
        spec("a", 64, 64, 11, 61),
        spec("b", 257, 257, 12, 180),
        spec("a", 4096, 4096, 13, 0),
        spec("b", 300, 300, 14, 180),  # beluga::estimate
        spec("b", 500, 2000, 15, 259),
        spec("a", 301, 301, 16, 180, sensor=LF_PROB),
        spec("b", 300, 300, 17, 180, motion=OMNI),
    ]
    fleet = cluster_fleet(worlds, specs, kind0=(3,))
    cycles = 4
    for _ in range(cycles):
        out = fleet.step()
        assert all(o is not None for o in out)
        for member, twin in zip(fleet.batch.members, fleet.twins):
            assert member.counter("cluster_cells") == twin.counter("cluster_cells")
    assert fleet.batch.counter("members_cluster_fused") == 6 * cycles
    assert fleet.batch.counter("cluster_launches") == 2 * cycles
    assert fleet.batch.counter("kernel_launches") == 3 * cycles
    assert fleet.batch.counter("members_fused") == 7 * cycles and fleet.batch.counter("members_alone") == 0
    fleet.close()


def test_it_is_really_batched(worlds):
    """The cluster launches of a cycle do not depend on the number of members (a loop over the lone estimate passes everything else)."""
    per_cycle = []
    for members in (2, 9):
        fleet = cluster_fleet(worlds, [spec("ab"[i % 2], 300 + 50 * i, 300 + 50 * i, 50 + i, 61) for i in range(members)])
        for _ in range(3):
            before = fleet.batch.counter("cluster_launches")
            fleet.step()
            per_cycle.append(fleet.batch.counter("cluster_launches") - before)
        assert fleet.batch.counter("members_cluster_fused") == 3 * members
        fleet.close()
    assert per_cycle == [2] * 6, per_cycle


def test_no_winner_takes_the_overall_estimate(worlds):
    """64 particles a metre apart, each alone in its cell, and no resampling (resample_interval = 3, two cycles): no cluster holds more
    than one particle, so the estimate is the overall one (cluster_based_estimation.hpp:424-427).  The member's own estimate() afterwards
    takes its sums about another pivot (the estimate just reported), so the two agree to rounding: 64 terms of magnitude <= 5^2 m^2 in
    double, 64 * 25 * 2^-53 = 2e-13; the bound is 1e-10, as in test_two_blobs."""
    fleet = cluster_fleet(worlds, [
        spec("a", 400, 400, 21, 61),
        spec("a", 64, 64, 22, 61, motion=StationaryModelParam(), resample_interval=3),
        spec("b", 300, 300, 23, 61),
    ])
    gx, gy = np.meshgrid(np.arange(8.0) - 3.5, np.arange(8.0) - 3.5)
    states = np.stack([np.ones(64), np.zeros(64), gx.ravel(), gy.ravel()], axis=1)
    fleet.both(1, lambda f: f.set_particles(states, np.ones(64)))
    for _ in range(2):
        out = fleet.step()
        assert not fleet.batch.last_infos[1]["resampled"]
        assert fleet.batch.members[1].counter("cluster_cells") == 64
        overall = fleet.batch.members[1].estimate()
        fleet.twins[1].estimate()  # (the call moves the pivot of the next cycle's sums: the twin makes it too)
        assert np.allclose(out[1][0], overall[0], rtol=0, atol=1e-10) and np.allclose(out[1][1], overall[1], rtol=0, atol=1e-10)
    assert fleet.batch.counter("cluster_launches") == 4 and fleet.batch.counter("members_cluster_fused") == 6
    fleet.close()


def test_far_cluster_takes_its_second_pass(worlds):
    """A map at UTM scale and a set of two blobs, the smaller one first: set_particles puts the pivot on the first particle, the empty
    scan leaves the weights at one, so the winning cluster is the larger blob, 3 m from the pivot and a tenth of a metre wide - its sums
    are taken once more about its own mean, on the twin and on the member alike."""
    fleet = cluster_fleet(worlds, [spec("a", 300, 300, 31, 61), spec("utm", 500, 500, 32, 0), spec("b", 300, 300, 33, 61)])
    states, weights = two_blobs(fleet.worlds[1].start)
    states = states[::-1].copy()
    fleet.both(1, lambda f: f.set_particles(states, weights))
    for _ in range(3):
        out = fleet.step()
        assert out[1] is not None
        assert fleet.batch.members[1].counter("estimate_repivots") == fleet.twins[1].counter("estimate_repivots")
    assert fleet.batch.members[1].counter("estimate_repivots") > 0
    assert fleet.batch.counter("members_cluster_fused") == 9
    fleet.close()


def test_two_blobs(worlds):
    """One stationary update of a set of two blobs 3 m apart: the heavier cluster's estimate, as the member's own entry points give it for
    the set the cycle left.  Those take their sums about another pivot (the estimate just reported), so they agree to rounding: 500 terms
    of magnitude <= 3^2 m^2 in double, 500 * 9 * 2^-53 = 5e-13; the bound is 1e-10."""
    fleet = cluster_fleet(worlds, [spec("a", 500, 500, 41, 61, motion=StationaryModelParam()), spec("b", 300, 300, 42, 61)])
    start = fleet.worlds[0].start
    states, weights = two_blobs((start[0] - 1.5, start[1], start[2]))
    fleet.both(0, lambda f: f.set_particles(states, weights))
    out = fleet.step()
    pose, cov = out[0]
    later = fleet.batch.members[0].cluster_based_estimate()
    assert np.allclose(pose, later[0], rtol=0, atol=1e-10) and np.allclose(cov, later[1], rtol=0, atol=1e-10)
    total, clusters = fleet.batch.members[0].estimate_clusters()
    assert total >= 1
    assert np.allclose(pose, clusters[0][3], rtol=0, atol=1e-10) and np.allclose(cov, clusters[0][4], rtol=0, atol=1e-10)
    twin_later = fleet.twins[0].cluster_based_estimate()
    assert np.array_equal(later[0], twin_later[0]) and np.array_equal(later[1], twin_later[1])
    fleet.close()


def test_policies(worlds):
    """resample_interval = 2 (non-unit weights at every other estimate), a member that stands still in cycles 2 and 3, and a cycle in
    which no cluster-based member moves: no cluster launch."""
    fleet = cluster_fleet(worlds, [
        spec("a", 500, 500, 51, 61, resample_interval=2),
        spec("b", 300, 1000, 52, 61),
        spec("a", 300, 300, 53, 61),  # beluga::estimate
    ], kind0=(2,))
    counted = 0
    for c in range(5):
        still = {2: (1,), 3: (0, 1)}.get(c, ())
        before = fleet.batch.counter("cluster_launches")
        out = fleet.step(hold=still)
        for i in still:
            assert out[i] is None and not fleet.batch.last_infos[i]["updated"]
        counted += 2 - len(still)
        assert fleet.batch.counter("cluster_launches") - before == (0 if c == 3 else 2)
        assert fleet.batch.counter("members_cluster_fused") == counted
    assert fleet.batch.counter("kernel_launches") == 15
    fleet.close()


def test_members_that_run_alone(worlds):
    """The beam model and a set beyond 4096 particles, both cluster-based: their own mcl_cluster_based_estimate, inside their own cycle."""
    fleet = cluster_fleet(worlds, [
        spec("a", 400, 400, 61, 61),
        spec("a", 300, 300, 62, 61, sensor=BEAM),
        spec("b", 5000, 5000, 63, 61),
        spec("b", 257, 257, 64, 61),
    ])
    for _ in range(3):
        fleet.step()
    assert fleet.batch.counter("members_alone") == 6 and fleet.batch.counter("members_fused") == 6
    assert fleet.batch.counter("members_cluster_fused") == 6 and fleet.batch.counter("cluster_launches") == 6
    fleet.close()


def test_switch(worlds):
    """batch_cluster_fused = 0 on every member: each through its own kernels - equal to its twin and to a fleet with the option on."""
    specs = [spec("a", 400, 400, 71, 61), spec("b", 300, 900, 72, 61), spec("a", 257, 257, 73, 61)]
    off, on = cluster_fleet(worlds, specs), cluster_fleet(worlds, specs)
    off.batch.set_option("batch_cluster_fused", 0)
    on.batch.set_option("batch_cluster_fused", 1)
    for _ in range(3):
        a, b = off.step(), on.step()
        for x, y in zip(a, b):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
    assert off.batch.counter("cluster_launches") == 0 and off.batch.counter("members_cluster_fused") == 0
    assert off.batch.counter("members_fused") == 9 and off.batch.counter("kernel_launches") == 9
    assert on.batch.counter("cluster_launches") == 6 and on.batch.counter("members_cluster_fused") == 9
    with pytest.raises(capi.MclError) as e:
        off.batch.set_option("batch_cluster_fusion", 1)
    assert e.value.status == capi.MCL_ERR_INVALID_ARGUMENT
    off.close()
    on.close()
