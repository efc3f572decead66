"""The range table of the beam model on the device (mcl_build_range_table; include/beluga_mcl.h "Range table for the beam model") against
tests/range_table_reference.py, which tests/test_range_table_cpu.py holds to tests/raycast_reference.py and to its own mutants.

  1. The table, bit for bit: every grid of tests/beam_families.py, A in {1, 2, 63, 64, 65, 360}, the reference fed with the bearings the
     library used.  Small grids whole; of larger ones a fixed sample of rows (the reference walks cell by cell in Python), the device
     building the whole table all the same.  On identity-origin grids the table is also mcl_cast_rays from the cell centres.
  2. The weights: mcl_reweight, mcl_likelihoods and mcl_likelihoods_device over the table within the beam bar 1e-10
     (tests/test_gpu_beam_edges.py: libm in exp and erf) - after asserting ON THE REFERENCE ALONE that every (pose, beam) lies at
     least 1e-6 bins from a bin edge: the bin decision is only as exact as atan2.
  3. The table's own exact case: A = 4, heading 0, axis-aligned beams in a room - the table path is the exact path within 1e-10.
  4. The lifecycle: build and drop, the three ways a map is installed, the refusals, the counters, a member of a batch."""
import ctypes as C
import math

import numpy as np
import pytest

import beam_families as fam
import beam_reference as ref
import range_table_reference as rt
from beluga_amd import capi
from beluga_amd.amcl import (Amcl, AmclBatch, AmclParams, BeamModelParam, DifferentialDriveModelParam, LikelihoodFieldModelParam, OccupancyGrid,
                             SharedMap, se2_from_xytheta)

pytestmark = pytest.mark.gpu

MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
SMALL = AmclParams(min_particles=8, max_particles=8)
A_VALUES = (1, 2, 63, 64, 65, 360)
BAR = 1e-10
RES = fam.RES


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def grid_of(case):
    return OccupancyGrid(cells=case["cells"], resolution=case["resolution"], origin=case["origin"])


def beam_filter(case, max_range, params=SMALL, seed=11, **more):
    return Amcl(grid_of(case), MOTION, BeamModelParam(*ref.revealing_params(case["resolution"], max_range)), params, seed=seed, **more)


# ---- 1. the table -------------------------------------------------------------------------------------------------------------------------
def distinct_grids():
    """(family, case, max_range) per distinct (cells, origin, resolution) of the families: the largest max_range any of its cases has, and
    at least what crosses the grid where that stays below 2000 cells."""
    seen = {}
    for name in sorted(fam.FAMILIES):
        for case in fam.FAMILIES[name]():
            key = (id(case["cells"]), tuple(case["origin"]), case["resolution"])
            reach = float(case["params"][6])
            if key not in seen or reach > seen[key][2]:
                seen[key] = (name, case, max(reach, seen[key][2]) if key in seen else reach)
    out = []
    for name, case, reach in seen.values():
        H, W = case["cells"].shape
        across = (max(W, H) + 3.0) * case["resolution"]
        out.append((name, case, max(reach, across) if max(W, H) + 3 < 2000 else reach))
    return out


GRIDS = distinct_grids()


def sample_cells(W, H):
    """Every cell of a grid of up to 64; else the corners, the centre and a few fixed others - fewer on grids whose walks are long."""
    if W * H <= 64:
        return list(range(W * H))
    some = {0, W - 1, (H - 1) * W, W * H - 1, (H // 2) * W + W // 2}
    if W * H <= 200000:
        some |= {(H // 3) * W + (2 * W) // 3, (H - 2) * W + 1, W + W // 5}
    return sorted(some)


@pytest.mark.parametrize("k", range(len(GRIDS)), ids=["%s-%dx%d" % (g[0], g[1]["cells"].shape[1], g[1]["cells"].shape[0]) for g in GRIDS])
def test_the_table_equals_the_reference_on_every_grid_of_the_families(k):
    name, case, max_range = GRIDS[k]
    H, W = case["cells"].shape
    cells = sample_cells(W, H)
    identity = np.array_equal(case["origin"], fam.IDENTITY)
    f = beam_filter(case, max_range)
    try:
        for A in A_VALUES:
            f.build_range_table(A)
            info = f.range_table_info()
            assert (info["built"], info["num_angles"], info["width"], info["height"], info["bytes"]) == (1, A, W, H, W * H * A * 4)
            bearings = f.range_table_bearings()
            assert np.max(np.abs(bearings - rt.bearings_of(A))) <= 1e-15
            got = f.range_table().reshape(W * H, A)[cells] if W * H <= 64 else np.concatenate([f.range_table(c, 1) for c in cells])
            want = rt.table(case["cells"], case["resolution"], max_range, bearings, only_cells=cells)
            assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), want), (name, W, H, A)
            if identity:  # the exact caster from the cell centres, on more cells than the Python walk affords
                more = np.unique(np.concatenate([cells, (np.arange(500, dtype=np.int64) * 7919) % (W * H)]))
                poses = np.stack([np.ones(len(more)), np.zeros(len(more)), (more % W + 0.5) * case["resolution"], (more // W + 0.5) * case["resolution"]], axis=1)
                _, hits = f.cast_rays(poses, bearings=bearings, max_range=max_range, hit_cells=True)
                r2 = np.where(hits >= 0, np.minimum((hits % W - (more % W)[:, None]) ** 2 + (hits // W - (more // W)[:, None]) ** 2, rt.FARTHEST), rt.NO_HIT)
                rows = np.concatenate([f.range_table(int(c), 1) for c in more]) if W * H > 4096 else f.range_table().reshape(W * H, A)[more]
                assert np.array_equal(rows.astype(np.int64), r2), (name, W, H, A)
        assert f.range_table_info()["builds"] == len(A_VALUES)
    finally:
        f.close()


def test_a_workgroup_straddles_cells_and_a_launch_ends_mid_row():
    """257 x 130 cells x 65 bins: 256 entries are three cells and 61 bins of a fourth; launches of 100 workgroups (25 600 entries: 393 rows
    and 55 bins) end mid-row.  The table is the single launch's, and both are the reference's on the rows around the launch seams."""
    W, H, A = 257, 130, 65
    cells = fam.salt(H, W, 53)
    case = dict(cells=cells, resolution=RES, origin=fam.ROTATED)
    max_range = 300 * RES
    f = beam_filter(case, max_range)
    try:
        f.build_range_table(A)
        whole = f.range_table()
        f.set_option("range_table_launch", 25600)
        f.build_range_table(A)
        assert np.array_equal(f.range_table(), whole) and whole.shape == (H, W, A)
        seams = sorted({(c * 25600) // A + d for c in (1, 2, 50, 84) for d in (-1, 0, 1)} | {0, W * H - 1})
        want = rt.table(cells, RES, max_range, f.range_table_bearings(), only_cells=seams)
        assert np.array_equal(whole.reshape(W * H, A)[seams].astype(np.int64), want)
        assert (want == rt.NO_HIT).any() and ((want != rt.NO_HIT) & (want > 0)).any()
    finally:
        f.close()


# ---- 2. the weights -----------------------------------------------------------------------------------------------------------------------
A_W = 72
PARTICLE_COUNTS = (1, 63, 64, 65, 257, 16385)  # the last is above the ordered kernel's threshold
SCAN_SIZES = (1, 63, 64, 65, 129, 1081)
CAPACITY = max(PARTICLE_COUNTS)
HEAD_OFFSETS = (0.0, 0.49, -0.49, -0.25)
BEAM_OFFSETS = (0.0, 0.49, -0.49, 0.25)


def weight_case(reach_cells, points):
    """A salted 157 x 203 grid behind a rotated origin; twelve poses whose grid-frame headings sit at bin centres plus 0, +-0.49, -0.25
    bins, two of them outside the grid; beams at bin centres plus 0, +-0.49, +0.25 bins (no sum of the two lands on an edge)."""
    cells = fam.salt(157, 203)
    spots = [(20.3, 30.7), (101.5, 77.5), (150.2, 12.9), (60.6, 140.1), (199.9, 150.4), (5.5, 5.5), (88.8, 33.3), (170.1, 99.2), (44.4, 66.6),
             (120.7, 120.2), (-4.5, 50.5), (230.5, 170.5)]
    heads = [((7 * i + 3) % A_W + HEAD_OFFSETS[i % 4]) * (2.0 * math.pi / A_W) for i in range(len(spots))]
    states = np.array([fam.local_pose(fam.ROTATED, x, y, th) for (x, y), th in zip(spots, heads)])
    max_range = reach_cells * RES
    angles = [((5 * b + 1) % A_W + BEAM_OFFSETS[b % 4]) * (2.0 * math.pi / A_W) for b in range(points)]
    return dict(cells=cells, resolution=RES, origin=np.asarray(fam.ROTATED, dtype=np.float64), states=states,
                points=fam.scan(angles, fam.spread_ranges(points, min(max_range, 150 * RES), 0.05, 0.9)), params=ref.revealing_params(RES, max_range),
                targets="weights over the table, reach %d cells" % reach_cells)


def reference_weights(case, bearings):
    """rt.weights over a table that holds the reference's rows of the poses' source cells (no other row is read)."""
    H, W = case["cells"].shape
    b = rt.bins(case, A_W)
    source = sorted({int(y * W + x) for (x, y), inside in zip(b["source"], b["inside"]) if inside})
    table = np.full((W * H, A_W), rt.NO_HIT, dtype=np.int64)
    table[source] = rt.table(case["cells"], RES, float(case["params"][6]), bearings, only_cells=source)
    r = rt.weights(case, table, A_W)
    # asserted on the reference alone, before anything is compared: no (pose, beam) within 1e-6 bins of a bin edge
    assert r["margin"].min() >= 1e-6, r["margin"].min()
    assert (~r["inside"]).sum() == 2 and (r["r2"] != rt.NO_HIT).any() and (r["r2"][r["inside"]] == rt.NO_HIT).any()
    return r


@pytest.mark.parametrize("reach_cells", [120, 2100], ids=["beam_table", "no_beam_table"])
def test_reweight_and_likelihoods_over_the_table_match_the_reference(reach_cells):
    """reach 120 cells: the BeamTable arm; 2100 cells (> kBeamTableMaxCells = 2046) on the same small grid: a lane evaluates the entry itself."""
    import torch

    base = weight_case(reach_cells, max(SCAN_SIZES))
    f = beam_filter(base, float(base["params"][6]), AmclParams(min_particles=CAPACITY, max_particles=CAPACITY))
    try:
        f.build_range_table(A_W)
        bearings = f.range_table_bearings()
        w0 = np.random.Generator(np.random.MT19937(3)).uniform(0.5, 1.5, CAPACITY)
        for B in SCAN_SIZES:
            case = fam.prefix(base, B)
            r = reference_weights(case, bearings)
            for n in PARTICLE_COUNTS:
                idx = fam.assignment(case, CAPACITY)
                f.set_particles(case["states"][idx], w0)
                f.set_num_particles(n)
                before, visited = f.range_table_info()["lut_launches"], f.beam_cells_visited(reset=True)
                walked = {c: f.counter(c) for c in ("beam_wave_launches", "beam_ordered_launches")}
                f.reweight(case["points"])
                assert f.range_table_info()["lut_launches"] == before + 1 and f.beam_cells_visited() == 0
                assert walked == {c: f.counter(c) for c in walked}
                f.set_num_particles(CAPACITY)
                got = f.particles()[1]
                assert np.array_equal(got[n:], w0[n:]), "weights past n were written"
                want = r["weights"][idx[:n]] * w0[:n]
                err = float(np.max(np.abs(got[:n] - want) / want))
                like = f.likelihoods(case["states"][idx[:n]], case["points"])
                err_l = float(np.max(np.abs(like - r["weights"][idx[:n]]) / r["weights"][idx[:n]]))
                print("range_table reach=%d B=%d n=%d worst reweight %.3g likelihoods %.3g" % (reach_cells, B, n, err, err_l))
                assert err <= BAR and err_l <= BAR, (reach_cells, B, n, err, err_l)
                if n in (65, 16385):
                    d = f.likelihoods_device(torch.from_numpy(np.ascontiguousarray(case["states"][idx[:n]])).to("cuda:0"), case["points"])
                    assert np.array_equal(bits(d.cpu().numpy()), bits(like)), (reach_cells, B, n)
        f.set_option("beam_table", 0)  # (no BeamTable by the option either: the same bits)
        case = fam.prefix(base, 129)
        again = f.likelihoods(case["states"], case["points"])
        f.set_option("beam_table", 1)
        assert np.array_equal(bits(again), bits(f.likelihoods(case["states"], case["points"])))
    finally:
        f.close()


# ---- 3. the table's own exact case ----------------------------------------------------------------------------------------------------------
def test_with_four_bins_heading_zero_and_axis_aligned_beams_the_table_path_is_the_exact_path():
    W, H = 61, 47
    cells = np.zeros((H, W), dtype=np.int8)
    cells[0, :] = cells[-1, :] = cells[:, 0] = cells[:, -1] = ref.OCCUPIED
    case = dict(cells=cells, resolution=RES, origin=fam.IDENTITY)
    max_range = 100 * RES
    rng = np.random.Generator(np.random.MT19937(9))
    n = 257
    states = np.stack([np.ones(n), np.zeros(n), rng.uniform(1.1, W - 1.1, n) * RES, rng.uniform(1.1, H - 1.1, n) * RES], axis=1)
    # (measured ranges that are no multiple of the resolution: ON one, `measured < expected` is a tie that the exact path re-derives from the
    # two cell centres and the table path, which knows no hit cell, decides on sqrt(r2) * resolution - the one stated difference)
    points = np.array([[0.83, 0.0], [0.0, 1.37], [-2.21, 0.0], [0.0, -0.41], [1.91, 0.0], [0.0, 2.63], [-0.31, 0.0], [0.0, -1.73]])
    assert (np.abs(np.abs(points).sum(axis=1) / RES - np.round(np.abs(points).sum(axis=1) / RES)) > 0.1).all()
    w0 = rng.uniform(0.5, 1.5, n)
    params = AmclParams(min_particles=n, max_particles=n)
    table, exact = beam_filter(case, max_range, params), beam_filter(case, max_range, params)
    try:
        table.build_range_table(4)
        tcase = dict(case, states=states, points=points, params=ref.revealing_params(RES, max_range))
        assert rt.bins(tcase, 4)["margin"].min() >= 0.49  # (every beam at a bin centre)
        for f in (table, exact):
            f.set_particles(states, w0)
            f.reweight(points)
        got, want = table.particles()[1], exact.particles()[1]
        err = float(np.max(np.abs(got - want) / want))
        print("range_table exact case: worst %.3g" % err)
        assert err <= BAR
        assert np.max(np.abs(table.likelihoods(states, points) - exact.likelihoods(states, points)) / exact.likelihoods(states, points)) <= BAR
        assert table.range_table_info()["lut_launches"] == 1 and exact.range_table_info()["built"] == 0
    finally:
        table.close()
        exact.close()


# ---- 4. the lifecycle -----------------------------------------------------------------------------------------------------------------------
def room(W=90, H=67, pillar=(30, 25)):
    cells = np.zeros((H, W), dtype=np.int8)
    cells[0, :] = cells[-1, :] = cells[:, 0] = cells[:, -1] = ref.OCCUPIED
    cells[pillar[1]:pillar[1] + 4, pillar[0]:pillar[0] + 3] = ref.OCCUPIED
    return cells


ROOM_A = OccupancyGrid(cells=room(), resolution=RES, origin=se2_from_xytheta(-1.0, -0.5, 0.2))
ROOM_B = OccupancyGrid(cells=room(75, 81, (50, 60)), resolution=RES, origin=se2_from_xytheta(0.5, -1.5, -0.4))
BEAM = BeamModelParam(0.5, 0.5, 0.05, 0.05, 0.2, 0.1, 3.0)
LF = LikelihoodFieldModelParam(max_obstacle_distance=1.0, max_laser_distance=100.0, z_hit=0.5, z_random=0.5, sigma_hit=0.2)
CYCLE = AmclParams(min_particles=300, max_particles=600, update_min_d=0.0, update_min_a=0.0, resample_interval=1)
SCAN = fam.scan(2 * np.pi * np.arange(61) / 61 + 0.01, 0.4 + 1.9 * ((np.arange(61) * 0.618) % 1.0))


def start(f, grid=ROOM_A):
    f.initialize(np.array([grid.origin[2] + 1.5, grid.origin[3] + 1.2, 0.3]), np.diag([0.05, 0.05, 0.02]))


def cycles(filters, count, first=0):
    odom = (0.02 * first, 0.0, 0.01 * first)
    for c in range(first, first + count):
        odom = (odom[0] + 0.02, 0.0, odom[2] + 0.01)
        results = [f.update(se2_from_xytheta(*odom), SCAN) for f in filters]
        for r in results[1:]:
            assert (r is None) == (results[0] is None)
            if r is not None:
                assert np.array_equal(bits(r[0]), bits(results[0][0])) and np.array_equal(bits(r[1]), bits(results[0][1])), c
        for f in filters[1:]:
            assert f.particles()[0].tobytes() == filters[0].particles()[0].tobytes() and f.particles()[1].tobytes() == filters[0].particles()[1].tobytes(), c


def table_rows(f, grid, cells):
    want = rt.table(grid.cells, grid.resolution, BEAM.beam_max_range, f.range_table_bearings(), only_cells=cells)
    got = np.concatenate([f.range_table(int(c), 1) for c in cells])
    return got.astype(np.int64), want


def test_build_then_drop_leaves_the_bits_of_a_twin_that_never_built():
    built, twin = (Amcl(ROOM_A, MOTION, BEAM, CYCLE, seed=5) for _ in range(2))
    try:
        for f in (built, twin):
            start(f)
        cycles([built, twin], 2)
        built.build_range_table(90)
        assert built.range_table_info()["built"] == 1
        built.drop_range_table()
        info = built.range_table_info()
        assert (info["built"], info["num_angles"], info["bytes"], info["builds"], info["lut_launches"]) == (0, 0, 0, 1, 0)
        built.drop_range_table()  # (MCL_OK without a table)
        cycles([built, twin], 5, first=2)
        assert built.counter("beam_wave_launches") == twin.counter("beam_wave_launches") == 7
    finally:
        built.close()
        twin.close()


def test_every_way_to_install_a_map_rebuilds_the_table_of_the_new_map():
    f = Amcl(ROOM_A, MOTION, BEAM, CYCLE, seed=5)
    shared = SharedMap(ROOM_A, BEAM)
    try:
        start(f)
        f.build_range_table(40)
        cells_a, cells_b = [0, 91, 67 * 90 - 1, 33 * 90 + 45], [0, 76, 81 * 75 - 1, 40 * 75 + 37]
        got, want = table_rows(f, ROOM_A, cells_a)
        assert np.array_equal(got, want)
        steps = (("mcl_set_map", lambda: f.update_map(ROOM_B), ROOM_B, cells_b),
                 ("mcl_use_shared_map", lambda: f.use_map(shared), ROOM_A, cells_a),
                 ("async commit", lambda: (f.update_map_async(ROOM_B), f.map_commit(wait=True)), ROOM_B, cells_b))
        for k, (how, install, grid, cells) in enumerate(steps):
            install()
            info = f.range_table_info()
            H, W = grid.cells.shape
            assert (info["built"], info["num_angles"], info["width"], info["height"], info["builds"]) == (1, 40, W, H, 2 + k), how
            got, want = table_rows(f, grid, cells)
            assert np.array_equal(got, want), how
        # ... and between two updates, inside mcl_update
        f.update_map_async(ROOM_A)
        while f.map_pending() != 2:
            pass
        before = f.range_table_info()
        f.update(se2_from_xytheta(0.05, 0.0, 0.0), SCAN)
        info = f.range_table_info()
        assert info["builds"] == before["builds"] + 1 and (info["width"], info["height"]) == (90, 67) and info["lut_launches"] == before["lut_launches"] + 1
        got, want = table_rows(f, ROOM_A, cells_a)
        assert np.array_equal(got, want)
    finally:
        f.close()
        shared.close()


def test_refusals_leave_the_filter_and_the_table_untouched():
    lib = capi.load()
    f, lf = Amcl(ROOM_A, MOTION, BEAM, CYCLE, seed=5), Amcl(ROOM_A, MOTION, LF, CYCLE, seed=5)
    try:
        for g in (f, lf):
            start(g)
        assert lib.mcl_build_range_table(lf._ctx, 360) == capi.MCL_ERR_INVALID_ARGUMENT and lf.range_table_info()["built"] == 0
        assert lib.mcl_build_range_table(None, 360) == capi.MCL_ERR_INVALID_ARGUMENT
        out = np.zeros(16, dtype=np.uint32)
        assert lib.mcl_range_table_read(f._ctx, 0, 1, out.ctypes.data_as(capi.c_u32_p)) == capi.MCL_ERR_NOT_READY
        assert lib.mcl_range_table_bearings(f._ctx, np.zeros(8).ctypes.data_as(capi.c_double_p)) == capi.MCL_ERR_NOT_READY
        f.build_range_table(16)
        info, whole, particles = f.range_table_info(), f.range_table(), f.particles()
        f.set_option("range_table_max_bytes", 90 * 67 * 32 * 4 - 1)
        for A, status in ((0, capi.MCL_ERR_INVALID_ARGUMENT), (4097, capi.MCL_ERR_INVALID_ARGUMENT), (32, capi.MCL_ERR_OUT_OF_MEMORY)):
            assert lib.mcl_build_range_table(f._ctx, A) == status, A
            assert f.range_table_info() == info and np.array_equal(f.range_table(), whole)
            assert f.particles()[0].tobytes() == particles[0].tobytes() and f.particles()[1].tobytes() == particles[1].tobytes()
        assert lib.mcl_range_table_read(f._ctx, 90 * 67, 1, out.ctypes.data_as(capi.c_u32_p)) == capi.MCL_ERR_INVALID_ARGUMENT
        assert lib.mcl_range_table_read(f._ctx, 2 ** 64 - 1, 2, out.ctypes.data_as(capi.c_u32_p)) == capi.MCL_ERR_INVALID_ARGUMENT
        assert lib.mcl_range_table_read(f._ctx, 90 * 67 - 1, 1, out.ctypes.data_as(capi.c_u32_p)) == capi.MCL_OK
        assert np.array_equal(out, whole[-1, -1])
        f.set_option("range_table_max_bytes", 90 * 67 * 32 * 4)
        f.build_range_table(32)  # at the cap: built, and it replaces the table of 16 bins
        assert f.range_table_info()["num_angles"] == 32 and f.range_table_info()["builds"] == 2
    finally:
        f.close()
        lf.close()


def test_the_cycle_over_the_table_counts_one_launch_a_reweight_and_walks_no_cell():
    f, exact = Amcl(ROOM_A, MOTION, BEAM, CYCLE, seed=5), Amcl(ROOM_A, MOTION, BEAM, CYCLE, seed=5)
    try:
        for g in (f, exact):
            start(g)
        f.build_range_table(360)
        f.beam_cells_visited(reset=True)
        exact.beam_cells_visited(reset=True)
        for c in range(4):
            for g in (f, exact):
                g.update(se2_from_xytheta(0.02 * (c + 1), 0.0, 0.01 * (c + 1)), SCAN)
        assert f.range_table_info()["lut_launches"] == 4 and f.beam_cells_visited() == 0 and exact.beam_cells_visited() > 0
        assert f.counter("beam_wave_launches") == 0 and f.counter("beam_ordered_launches") == 0 and exact.counter("beam_wave_launches") == 4
        # the search and the caster stay exact: the same hits and ranges with and without a table
        poses = exact.particles()[0][:50]
        assert np.array_equal(bits(f.cast_rays(poses, points=SCAN)), bits(exact.cast_rays(poses, points=SCAN)))
        a, b = f.global_search(SCAN), exact.global_search(SCAN)
        assert len(a) > 0 and [(h.id, h.score) for h in a] == [(h.id, h.score) for h in b]
    finally:
        f.close()
        exact.close()


def test_a_member_of_a_batch_with_a_table_is_the_same_filter_updated_alone():
    params = AmclParams(min_particles=200, max_particles=400, update_min_d=0.0, update_min_a=0.0, resample_interval=1)
    specs = [dict(grid=ROOM_A, motion=MOTION, sensor=BEAM, params=params, seed=30 + k, options={"batch_beam_fused": 1}) for k in range(3)]
    fleet = AmclBatch(specs)
    lone = Amcl(ROOM_A, MOTION, BEAM, params, seed=31, options={"batch_beam_fused": 1})
    try:
        for m in list(fleet.members) + [lone]:
            start(m)
        fleet.members[1].build_range_table(90)
        lone.build_range_table(90)
        odom = (0.0, 0.0, 0.0)
        for c in range(4):
            odom = (odom[0] + 0.02, 0.0, odom[2] + 0.01)
            got = fleet.update([se2_from_xytheta(*odom)] * 3, [SCAN] * 3)[1]
            want = lone.update(se2_from_xytheta(*odom), SCAN)
            assert (got is None) == (want is None)
            if got is not None:
                assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), c
            a, b = fleet.members[1].particles(), lone.particles()
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), c
        assert fleet.members[1].range_table_info()["lut_launches"] == 4 and fleet.members[0].range_table_info()["lut_launches"] == 0
        assert fleet.members[0].beam_cells_visited() > 0 and fleet.members[1].beam_cells_visited() == 0
    finally:
        fleet.close()
        lone.close()
