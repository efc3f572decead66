"""Options draw_key_hist and rows_merged: the draw kernel counts the high digit of the keys it predicts for the next cycle's order (half-column
histograms, a draw workgroup covering 1024 slots = half a chunk of the ordering's table) instead of k_key_hist reading the keys back, and
the row scan over those counts runs in the launch of k_final_rows.  Only integer counts change hands and unchanged code runs in another grid:
with either option on or off, every particle, weight, estimate, covariance and counter is the same bit for bit."""
import functools
import os

import numpy as np
import pytest

from beluga_amd import synth
from beluga_amd.amcl import (Amcl, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam, OccupancyGrid,
                             se2_from_xytheta)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CYCLES, BEAMS, MAX_RANGE = 5, 64, 3.5
DRAW_SLOTS, CHUNK = 1024, 2048  # kDrawBlock, kChunk (kernels.hip, kernels.h)
# the first size on the large path; a last draw workgroup of one slot that opens a table column alone; whole columns only; a last column
# of one slot; two to the seventeenth
SIZES = [65_537, 65 * DRAW_SLOTS + 1, 33 * CHUNK, 34 * CHUNK + 1, 131_072]
SETTINGS = [(0, 0), (1, 0), (0, 1), (1, 1)]  # (draw_key_hist, rows_merged); the first is the reference


@functools.lru_cache(maxsize=None)
def workload(jump):
    """-> (grid, truth, [(control, points)]): a constant control action; jump: cycle 3's is far from the one predicted for it."""
    z = np.load(os.path.join(GOLDEN, "turtlebot3_world_grid.npz"))
    cells, res = z["cells"], float(z["resolution"])
    ox, oy, ot = z["origin_xytheta"]
    grid = OccupancyGrid(cells=cells, resolution=res, origin=se2_from_xytheta(ox, oy, ot))
    truth = synth.find_free_pose(cells, res, (ox, oy), seed=4, clearance_cells=8)
    angles = synth.lidar_angles(BEAMS, 360.0)
    pose, odom, steps = truth, (0.0, 0.0, 0.0), []
    for c in range(CYCLES):
        pose = synth.odometry_step(pose, 0.3, 0.05)
        odom = synth.odometry_step(odom, 0.3, 0.05)
        if jump and c == 3:  # sideways and turned (the scans stay what they are: the weights do not care)
            odom = (odom[0] + 0.35, odom[1] - 0.4, odom[2] + 0.6)
        ranges = synth.cast_scan(cells, res, (ox, oy), pose, angles, MAX_RANGE, 0.01, seed=100 + c)
        steps.append((se2_from_xytheta(*odom), synth.scan_points(ranges, angles)))
    return grid, truth, steps


def run(n, setting, jump=False):
    """-> (per cycle: pose, covariance, weight sum, particles, weights; counters)"""
    grid, truth, steps = workload(jump)
    f = Amcl(grid, DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05), LikelihoodFieldModelParam(2.0, 100.0, 0.5, 0.5, 0.2, True),
             AmclParams(min_particles=n, max_particles=n), seed=0xBE1A6A)
    f.set_option("cycle_spin", 1)  # (the order ahead belongs to cycles that end on the completion word: by default from 256K particles on)
    f.set_option("draw_key_hist", setting[0])
    f.set_option("rows_merged", setting[1])
    f.initialize(truth, np.diag([0.25, 0.25, 0.04]))
    cycles = []
    for control, points in steps:
        e = f.update(control, points)
        assert e is not None and f.last_info["resampled"]
        states, weights = f.particles()
        cycles.append((np.array(e[0]), np.array(e[1]), f.last_info["weight_sum"], states.copy(), weights.copy()))
    counters = {k: f.counter(k) for k in ("order_ahead_used", "order_ahead_missed", "noise_ahead_used", "lf_patch_groups_planned",
                                          "lf_patch_groups_through")}
    f.close()
    return cycles, counters


def assert_same(ref, other, what):
    (ref_cycles, ref_counters), (cycles, counters) = ref, other
    assert counters == ref_counters, (what, counters, ref_counters)
    for c, (a, b) in enumerate(zip(ref_cycles, cycles)):
        for name, x, y in zip(("pose", "covariance", "weight sum", "particles", "weights"), a, b):
            assert np.array_equal(x, y), (what, "cycle", c, name)


@pytest.mark.parametrize("n", SIZES)
def test_counts_from_the_draw_and_the_merged_launch_leave_every_bit(n):
    """A steady trajectory: a prediction after every cycle; the first real motion is predicted from the filter's motionless first update and
    refused, every later one is used - else the order computed from the draw's counts would never reach a result."""
    ref = run(n, SETTINGS[0])
    print(n, ref[1])
    assert ref[1]["order_ahead_used"] + ref[1]["order_ahead_missed"] == CYCLES - 1 and ref[1]["order_ahead_used"] >= CYCLES - 2, ref[1]
    for setting in SETTINGS[1:]:
        assert_same(ref, run(n, setting), setting)


def test_a_refused_order_falls_back_to_the_real_poses_with_the_same_bits():
    """Cycle 3's control action is far from the predicted one: the order (and the table the draw's counts went into) is dropped, the cycle
    orders by the real poses - k_propagate's keys and whole-column histograms in the same table."""
    n = SIZES[1]
    ref = run(n, SETTINGS[0], jump=True)
    print(n, ref[1])
    assert ref[1]["order_ahead_used"] >= 1 and ref[1]["order_ahead_missed"] >= 2, ref[1]
    for setting in SETTINGS[1:]:
        assert_same(ref, run(n, setting, jump=True), setting)
