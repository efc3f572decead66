"""What a context, a shared map and a batch give back when they are destroyed.  Every buffer of mcl_ctx, MapStore and mcl_batch is a
member that frees itself (DeviceBuffer, HostBuffer: map_store.h), and mcl_destroy / mcl_batch_destroy only do what a member's destructor
cannot; here one owner of every kind lives and dies, twice over, and the device's free memory must come back.  In the same file: the
option and counter names - public strings - are pinned and every one of them is accepted."""
import ctypes as C

import numpy as np
import pytest
import torch

from beluga_amd import capi
from beluga_amd.amcl import (Amcl, AmclBatch, AmclParams, BeamModelParam, DifferentialDriveModelParam, LandmarkMap, LandmarkMapBoundaries,
                             LandmarkModelParam, LandmarkPositionDetection, LikelihoodFieldModelParam, NDTMap2d, NDTModelParam2d,
                             OccupancyGrid, SharedMap, se2_from_xytheta)
from test_options_host_cpu import OPTION_NAMES

pytestmark = pytest.mark.gpu

COUNTER_NAMES = [
    "lf_fast_launches", "lf_patch_launches", "lf_queue_launches", "lf_beams_launches", "lf_far_launches", "lf_far_beams_launches",
    "small_tail_launches", "estimate_repivots", "lf_far_tiles", "noise_ahead_used", "order_ahead_used", "order_ahead_missed",
    "lf_patch_groups_planned", "lf_patch_groups_through", "host_ns_to_first_launch", "host_ns_other_launches", "host_ns_wait",
    "host_ns_after_wait", "host_cycles", "field_build_us", "field_built_on_device", "map_device_bytes", "map_shared", "cluster_cells",
    "comm_bytes_out", "comm_collectives", "comm_host_syncs", "comm_overflows", "comm_ranks_seen", "comm_backend"]
BATCH_COUNTER_NAMES = ["cycles", "kernel_launches", "members_fused", "members_alone", "cluster_launches", "members_cluster_fused",
                       "cluster_host_ns", "beam_launches", "members_beam_fused"]

# The device allocator hands memory out in granules of 2 MiB (the driver's large page): the finest step free memory moves in.
GRANULE = 2 << 20

N = 512
MOTION = DifferentialDriveModelParam(0.1, 0.1, 0.1, 0.1)
PARAMS = AmclParams(min_particles=N, max_particles=N)
CONTROLS = [se2_from_xytheta(0.0, 0.0, 0.0), se2_from_xytheta(0.3, 0.0, 0.1)]  # the first update is forced, the second has moved


def small_grid():
    cells = np.zeros((32, 32), dtype=np.int8)
    cells[0, :] = cells[-1, :] = cells[:, 0] = cells[:, -1] = 100
    cells[12:15, 20:23] = 100
    return OccupancyGrid(cells=cells, resolution=0.1)


def scan8():
    a = np.linspace(-np.pi, np.pi, 8, endpoint=False)
    return np.stack([1.2 * np.cos(a), 1.2 * np.sin(a)], axis=1)


def live_and_die(f, measurements):
    f.initialize((1.6, 1.6, 0.0), np.diag([0.04, 0.04, 0.01]))
    for control, m in zip(CONTROLS, measurements):
        f.update(control, m)
    pose, _ = f.cluster_based_estimate()
    assert np.all(np.isfinite(pose))
    f.close()


def case_grid(sensor):
    live_and_die(Amcl(small_grid(), MOTION, sensor, PARAMS, seed=3), [scan8(), scan8()])


def case_ndt():
    keys = np.array([[x, y] for x in range(4) for y in range(4)], dtype=np.int32)  # 16 cells
    ndt = NDTMap2d(keys, keys + 0.5, np.tile(np.eye(2) * 0.05, (16, 1, 1)), 1.0)
    live_and_die(Amcl(ndt, MOTION, NDTModelParam2d(), PARAMS, seed=3), [scan8() + 1.6, scan8() + 1.6])


def case_landmarks():
    entries = [LandmarkPositionDetection((x, y, 0.0), c) for (x, y), c in zip([(0.5, 0.5), (2.5, 0.5), (0.5, 2.5), (2.5, 2.5)], [1, 2, 1, 3])]
    lmap = LandmarkMap(LandmarkMapBoundaries((0.0, 0.0, 0.0), (3.2, 3.2, 0.0)), entries)
    seen = [LandmarkPositionDetection((1.0, 1.0, 0.0), 1), LandmarkPositionDetection((-1.0, 1.0, 0.0), 2)]
    live_and_die(Amcl(lmap, MOTION, LandmarkModelParam(), PARAMS, seed=3), [seen, seen])


def case_shared_map(release_first):
    shared = SharedMap(small_grid(), LikelihoodFieldModelParam())
    readers = []
    for s in (3, 4):
        f = Amcl.__new__(Amcl)
        cfg = f._configure(None, MOTION, LikelihoodFieldModelParam(), PARAMS, seed=s)
        ctx = capi._ctx()
        assert f._lib.mcl_create(C.byref(cfg), C.byref(ctx)) == capi.MCL_OK
        f._attach(ctx, None, None, owned=True)
        f.use_map(shared)
        readers.append(f)
    if release_first:
        shared.close()  # (the store lives on while a context reads it)
    for f in readers:
        live_and_die(f, [scan8(), scan8()])
    if not release_first:
        shared.close()


def case_batch():
    grid = small_grid()
    batch = AmclBatch([dict(grid=grid, motion=MOTION, sensor=LikelihoodFieldModelParam(), params=PARAMS, seed=s) for s in (3, 4, 5)])
    batch.members[1].set_estimate_kind(True)
    for member in batch.members:
        member.initialize((1.6, 1.6, 0.0), np.diag([0.04, 0.04, 0.01]))
    for control in CONTROLS:
        batch.update([control] * 3, [scan8()] * 3)
    for name in BATCH_COUNTER_NAMES:
        assert batch.counter(name) >= 0
    assert batch.counter("cycles") == 2
    with pytest.raises(capi.MclError, match="mcl_batch_get_counter: unknown counter no_such_counter"):
        batch.counter("no_such_counter")
    batch.close()  # (mcl_destroy on a former member's pointer is not called: the batch was the owner)


def case_collective_option():
    f = Amcl(small_grid(), MOTION, LikelihoodFieldModelParam(), PARAMS, seed=3)
    assert f._lib.mcl_comm_attach(f._ctx, 0, 1, None) == capi.MCL_OK  # the in-process transport: a world of one
    f.set_option("device_policy", 0)
    f.set_option("shard_pad_permille", 500)
    live_and_die(f, [scan8(), scan8()])


def every_owner_once():
    case_grid(LikelihoodFieldModelParam())
    case_grid(BeamModelParam())
    case_ndt()
    case_landmarks()
    case_shared_map(release_first=True)
    case_shared_map(release_first=False)
    case_batch()
    case_collective_option()


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_every_owner_gives_its_memory_back():
    """Measured on an MI355X: the first time a process runs the sequence, free memory falls by what the HIP runtime takes once and keeps - the
    code objects of the kernels it meets, its pools: 160 MiB in a fresh process, 4 MiB in one that had run the rest of the suite, and
    nothing on the next pass in either.  So the sequence runs once before the first reading; from there on nothing may be lost."""
    capi.load()
    every_owner_once()
    before = free_bytes()
    every_owner_once()
    after_first = free_bytes()
    every_owner_once()
    after_second = free_bytes()
    print("free bytes before %d, after the first pass %d (%+d), after the second %d (%+d)"
          % (before, after_first, after_first - before, after_second, after_second - after_first))
    assert after_first >= before - GRANULE
    assert after_second >= after_first


def test_every_option_and_counter_name_is_accepted():
    f = Amcl(small_grid(), MOTION, LikelihoodFieldModelParam(), PARAMS, seed=3)
    try:
        for name in OPTION_NAMES:
            f.set_option(name, 1)
        for name in COUNTER_NAMES:
            assert f.counter(name) >= 0
        with pytest.raises(capi.MclError, match="mcl_set_option: unknown option no_such_option"):
            f.set_option("no_such_option", 1)
        with pytest.raises(capi.MclError, match="mcl_get_counter: unknown counter no_such_counter"):
            f.counter("no_such_counter")
    finally:
        f.close()
