"""mcl_shared_map_* / mcl_use_shared_map: one uploaded map read by many filters (DESIGN.md "Shared maps").

The yardstick is the one of test_gpu_batch.py: every filter attached to a shared map has a TWIN that was given the same grid through
mcl_set_map, and after every cycle the estimate, every field of mcl_update_info, the particle states, the weights and the count are
compared with np.array_equal.  The maps are 101 x 75 and 90 x 67 cells - off the 8 x 8 tile on both axes, so the border tiles are live."""
import numpy as np
import pytest

from beluga_amd import capi, synth
from beluga_amd.amcl import (Amcl, AmclParams, NDTMap2d, NDTModelParam2d, OccupancyGrid, SharedMap, LikelihoodFieldModelParam,
                             se2_from_xytheta)
from test_gpu_batch import BEAM, COV, LF_PROB, Fleet, World, spec, wide_grid
from test_gpu_parity import LF, MOTION
from test_shared_map_cpu import compile_driver, store_bytes

pytestmark = pytest.mark.gpu

BEAMS = 61


def odd_grid(width, height, seed):
    cells = synth.make_rooms_map(width, height, seed=seed, n_rooms=3)
    return OccupancyGrid(cells=cells, resolution=0.05, origin=se2_from_xytheta(-2.5, -1.9, 0.0))


@pytest.fixture(scope="module")
def worlds():
    return {"a": World(odd_grid(101, 75, 5)), "b": World(wide_grid()), "other": World(odd_grid(90, 67, 8))}


@pytest.fixture(scope="module")
def bytes_driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("map_store_bytes"), "driver")


def attach(fleet, shared, members=None):
    for i in (range(len(fleet.batch.members)) if members is None else members):
        fleet.batch.members[i].use_map(shared)


SIX = [("a", 300, 500, 11), ("a", 400, 400, 12), ("a", 300, 300, 13), ("a", 350, 500, 14), ("a", 500, 500, 15), ("a", 300, 450, 16)]


@pytest.mark.parametrize("case", ["lf", "lf_prob", "cluster_based"])
def test_attached_members_equal_privately_mapped_twins(worlds, case):
    """Six members - KLD 300..500 and fixed sizes, their own seeds - read one store; their twins each hold the same grid privately."""
    sensor = LF_PROB if case == "lf_prob" else LF
    fleet = Fleet(worlds, [spec(w, lo, hi, seed, BEAMS, sensor=sensor) for w, lo, hi, seed in SIX])
    if case == "cluster_based":
        for i in range(len(SIX)):
            fleet.both(i, lambda f: f.set_estimate_kind(cluster_based=True))
    shared = SharedMap(worlds["a"].grid, sensor)
    attach(fleet, shared)
    assert shared.info()["users"] == len(SIX)
    cycles = 5
    for _ in range(cycles):
        out = fleet.step()
        assert all(o is not None for o in out)
    assert fleet.batch.counter("members_fused") == cycles * len(SIX) and fleet.batch.counter("members_alone") == 0
    assert fleet.batch.counter("kernel_launches") == 3 * cycles
    for member in fleet.batch.members:
        assert member.counter("map_shared") == 1 and member.counter("map_device_bytes") == 0
    fleet.close()
    assert shared.info()["users"] == 0
    shared.close()


def test_large_path_member_reads_palette_patches_and_far_tiles(worlds):
    """5000 particles on the wide map: the ordered kernels of the large path, which read the palette, the far-tile bitmaps and the pz^3
    table of the store."""
    fleet = Fleet(worlds, [spec("b", 5000, 5000, 21, BEAMS)])
    shared = SharedMap(worlds["b"].grid, LF)
    attach(fleet, shared)
    member, twin = fleet.batch.members[0], fleet.twins[0]
    for _ in range(4):
        fleet.step()
    assert fleet.batch.counter("members_alone") == 4
    for name in ("lf_far_tiles", "lf_fast_launches", "lf_patch_launches", "lf_far_launches", "lf_beams_launches"):
        assert member.counter(name) == twin.counter(name), name
    fleet.close()
    shared.close()


def test_beam_member_reads_a_beam_store(worlds):
    fleet = Fleet(worlds, [spec("a", 300, 300, 31, BEAMS, sensor=BEAM), spec("a", 300, 500, 32, BEAMS)])
    beam_map, lf_map = SharedMap(worlds["a"].grid, BEAM), SharedMap(worlds["a"].grid, LF)
    attach(fleet, beam_map, [0])
    attach(fleet, lf_map, [1])
    info = beam_map.info()
    assert info["sensor_kind"] == capi.MCL_SENSOR_BEAM and info["host_bytes"] == 0 and info["users"] == 1
    for _ in range(4):
        fleet.step()
    assert fleet.batch.members[0].counter("map_shared") == 1
    fleet.close()
    beam_map.close()
    lf_map.close()


def test_two_lone_contexts_on_two_streams_read_one_store(worlds):
    world = worlds["a"]
    params = [AmclParams(min_particles=300, max_particles=500), AmclParams(min_particles=400, max_particles=400)]
    lone = [Amcl(world.grid, MOTION, LF, p, seed=41 + i) for i, p in enumerate(params)]  # (each creates a stream of its own)
    twins = [Amcl(world.grid, MOTION, LF, p, seed=41 + i) for i, p in enumerate(params)]
    shared = SharedMap(world.grid, LF)
    for f in lone:
        f.use_map(shared)
    for f in lone + twins:
        f.initialize(world.start, COV)
    assert shared.info()["users"] == 2
    for cycle in range(1, 5):
        for got_f, want_f in zip(lone, twins):
            got, want = got_f.update(world.odom(cycle), world.scan(cycle, BEAMS)), want_f.update(world.odom(cycle), world.scan(cycle, BEAMS))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            (gs, gw), (ws, ww) = got_f.particles(), want_f.particles()
            assert np.array_equal(gs, ws) and np.array_equal(gw, ww)
            assert got_f.last_info == want_f.last_info
    lone[0].close()
    assert shared.info()["users"] == 1
    for f in lone[1:] + twins:
        f.close()
    assert shared.info()["users"] == 0
    shared.close()


def test_random_states_and_global_localisation_draw_from_the_shared_free_cells(worlds):
    fleet = Fleet(worlds, [spec("a", 500, 500, 51, BEAMS), spec("a", 300, 500, 52, BEAMS)])
    shared = SharedMap(worlds["a"].grid, LF)
    attach(fleet, shared)
    for i in range(2):
        fleet.both(i, lambda f: f.initialize_from_map())
        fleet.compare(i, None, None)  # (the set drawn from the free cells)
    fleet.both(0, lambda f: f.debug_set_recovery_filters(1.0, 0.5))
    injected = False
    for _ in range(4):
        fleet.step()
        injected = injected or fleet.batch.last_infos[0]["random_state_probability"] > 0.0
    assert injected
    fleet.close()
    shared.close()


def test_swap_to_another_shared_map_mid_run(worlds):
    """At cycle 3 the members go from map a to the 90 x 67 map through mcl_use_shared_map, the twins through mcl_set_map; member 2 had a
    map on its way (mcl_set_map_async), which the new map replaces on both sides."""
    fleet = Fleet(worlds, [spec("a", 300, 500, 61, BEAMS), spec("a", 400, 400, 62, BEAMS), spec("a", 300, 300, 63, BEAMS)])
    first, second = SharedMap(worlds["a"].grid, LF), SharedMap(worlds["other"].grid, LF)
    attach(fleet, first)
    for cycle in range(5):
        if cycle == 3:
            fleet.both(2, lambda f: f.update_map_async(worlds["b"].grid))
            attach(fleet, second)
            for twin in fleet.twins:
                twin.update_map(worlds["other"].grid)
            fleet.both(2, lambda f: f.map_commit())
            for i in range(3):
                assert fleet.batch.members[i].map_pending() == 0 and fleet.twins[i].map_pending() == 0
                assert np.array_equal(fleet.batch.members[i].likelihood_field(), fleet.twins[i].likelihood_field())
            assert first.info()["users"] == 0 and second.info()["users"] == 3
        fleet.step()
    assert fleet.batch.members[0].likelihood_field().shape == (67, 90)
    fleet.close()
    first.close()
    second.close()


def test_ownership_bytes_release_and_detach(worlds, bytes_driver):
    world = worlds["a"]
    fleet = Fleet(worlds, [spec("a", 300, 500, 71, BEAMS), spec("a", 400, 400, 72, BEAMS), spec("a", 300, 300, 73, BEAMS)])
    private_bytes = [m.counter("map_device_bytes") for m in fleet.batch.members]
    assert all(m.counter("map_shared") == 0 for m in fleet.batch.members)
    shared = SharedMap(world.grid, LF)
    attach(fleet, shared)
    info = shared.info()
    assert (info["width"], info["height"], info["resolution"], info["sensor_kind"], info["device_id"]) == (101, 75, 0.05, 0, 0)
    assert info["users"] == 3
    # the bytes, against the accounting of map_store_host.cpp for what this map turns out to be
    field = fleet.twins[0].likelihood_field()
    unknown = np.float32(1.0 / LF.max_laser_distance)
    palette = len(np.unique(np.append(field.ravel().view(np.uint32), unknown.reshape(1).view(np.uint32))))
    n_free = int((np.asarray(world.grid.cells) == world.grid.value_traits[0]).sum())
    far = fleet.batch.members[0].counter("lf_far_tiles") != 0
    want = store_bytes(bytes_driver, capi.MCL_SENSOR_LIKELIHOOD_FIELD, 101, 75, n_free, 0, palette, far)
    assert (info["device_bytes"], info["host_bytes"]) == want
    assert private_bytes == [want[0]] * 3  # (a first private map is built from nothing as well)
    for member in fleet.batch.members:
        assert member.counter("map_shared") == 1 and member.counter("map_device_bytes") == 0
    fleet.step()
    # the handle goes while the members still read the map
    shared.close()
    for _ in range(2):
        fleet.step()
    # a member that takes a map of its own leaves the store (seen through a handle-free path: the others still run, and match)
    fleet.both(1, lambda f: f.update_map(worlds["other"].grid))
    assert fleet.batch.members[1].counter("map_shared") == 0 and fleet.batch.members[1].counter("map_device_bytes") > 0
    assert fleet.batch.members[0].counter("map_shared") == 1
    fleet.step()
    fleet.close()


def test_users_drop_when_a_member_detaches(worlds):
    fleet = Fleet(worlds, [spec("a", 300, 300, 75, BEAMS), spec("a", 300, 300, 76, BEAMS)])
    shared = SharedMap(worlds["a"].grid, LF)
    attach(fleet, shared)
    assert shared.info()["users"] == 2
    fleet.both(0, lambda f: f.update_map(worlds["a"].grid))
    assert shared.info()["users"] == 1 and fleet.batch.members[0].counter("map_device_bytes") > 0
    fleet.both(1, lambda f: f.update_map_async(worlds["other"].grid))
    fleet.both(1, lambda f: f.map_commit())  # the swap of an async map detaches as well
    assert shared.info()["users"] == 0
    fleet.step()
    fleet.close()
    shared.close()


def test_refusals_leave_the_context_alone(worlds):
    world = worlds["a"]
    fleet = Fleet(worlds, [spec("a", 300, 500, 81, BEAMS), spec("a", 300, 300, 82, BEAMS, sensor=BEAM)])
    shared = SharedMap(world.grid, LF)
    attach(fleet, shared, [0])
    other_lf = LikelihoodFieldModelParam(max_obstacle_distance=2.0, max_laser_distance=100.0, z_hit=0.5, z_random=0.5, sigma_hit=0.25,
                                         model_unknown_space=LF.model_unknown_space)
    wrong = {"sigma_hit": SharedMap(worlds["other"].grid, other_lf), "sensor_kind": SharedMap(worlds["other"].grid, LF_PROB),
             "beam": SharedMap(worlds["other"].grid, BEAM)}
    for word, bad in wrong.items():
        with pytest.raises(capi.MclError) as err:
            fleet.batch.members[0].use_map(bad)
        assert err.value.status == capi.MCL_ERR_INVALID_ARGUMENT and word in str(err.value)
        assert bad.info()["users"] == 0
    with pytest.raises(capi.MclError) as err:  # a likelihood-field map on the beam member
        fleet.batch.members[1].use_map(shared)
    assert err.value.status == capi.MCL_ERR_INVALID_ARGUMENT and "beam" in str(err.value)
    assert shared.info()["users"] == 1 and fleet.batch.members[0].likelihood_field().shape == (75, 101)
    # the store does not change: mcl_set_likelihood_field is refused and the field stays the twin's
    field = fleet.twins[0].likelihood_field()
    with pytest.raises(capi.MclError) as err:
        fleet.batch.members[0].set_likelihood_field(np.zeros_like(field))
    assert err.value.status == capi.MCL_ERR_UNSUPPORTED
    assert np.array_equal(fleet.batch.members[0].likelihood_field(), field)
    assert np.array_equal(fleet.batch.members[0].likelihood_field_origin(), fleet.twins[0].likelihood_field_origin())
    assert fleet.batch.members[0].has_likelihood_field()
    # an NDT context has a map of its own
    ndt = Amcl(NDTMap2d(np.array([[0, 0]], dtype=np.int32), np.array([[0.5, 0.5]]), np.array([[[0.1, 0.0], [0.0, 0.1]]]), 1.0), MOTION, NDTModelParam2d(), AmclParams(min_particles=100, max_particles=100), seed=1)
    with pytest.raises(capi.MclError) as err:
        ndt.use_map(shared)
    assert err.value.status == capi.MCL_ERR_UNSUPPORTED
    ndt.close()
    for _ in range(2):
        fleet.step()  # both members as their twins, after every refusal
    fleet.close()
    for bad in wrong.values():
        bad.close()
    shared.close()


def test_device_field_build_store_equals_a_private_device_build(worlds):
    """field_build = 1: the store's field by the device's distance transform, equal to what a context with that option builds."""
    world = worlds["a"]
    fleet = Fleet(worlds, [spec("a", 300, 500, 91, BEAMS, options={"field_build": 1})])
    shared = SharedMap(world.grid, LF, field_build=1)
    attach(fleet, shared)
    assert fleet.twins[0].counter("field_built_on_device") == 1 and fleet.batch.members[0].counter("field_built_on_device") == 1
    assert np.array_equal(fleet.batch.members[0].likelihood_field(), fleet.twins[0].likelihood_field())
    for _ in range(2):
        fleet.step()
    fleet.close()
    shared.close()
