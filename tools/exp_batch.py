"""Fleets of small filters: mcl_batch_update against a loop of mcl_update over the same members (DESIGN.md "Batched small filters").

    python tools/exp_batch.py [--fleets 1,4,16,64,256] [--cycles 40] [--rounds 7] [--json out.json]

Per fleet size F, two fleets on one small map: F filters of 2000 particles x 180 beams, fixed size, and the same KLD-adaptive
(500 .. 2000).  Both ways of updating alternate in one process on the same inputs: a timed round is `cycles` fleet updates through
mcl_batch_update, then `cycles` fleet updates by a loop of mcl_update over the members (the members are ordinary contexts, so the loop
is what a caller without the batch does).  One untimed round, then `rounds` timed ones; reported: wall time per fleet update (median,
minimum, maximum over the rounds), the per-filter quotient and the ratio batch : loop."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from beluga_amd import synth  # noqa: E402
from beluga_amd.amcl import (AmclBatch, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam, OccupancyGrid,  # noqa: E402
                             se2_from_xytheta)

MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
LF = LikelihoodFieldModelParam(2.0, 100.0, 0.5, 0.5, 0.2, True)
BEAMS = 180


def make_fleet(grid, members, lo, hi):
    specs = [dict(grid=grid, motion=MOTION, sensor=LF, params=AmclParams(min_particles=lo, max_particles=hi), seed=1000 + i)
             for i in range(members)]
    return AmclBatch(specs)


def drive(fleet, grid, start, cycles, first_cycle, by_batch):
    """`cycles` fleet updates from cycle number first_cycle on (the robot drives a circle: every update moves); seconds per fleet update."""
    n = len(fleet)
    origin = (grid.origin[2], grid.origin[3])
    angles = synth.lidar_angles(BEAMS, 270.0)
    inputs = []
    for c in range(first_cycle, first_cycle + cycles):
        pose, odom = start, (0.0, 0.0, 0.0)
        for _ in range(c % 7 + 1):  # (seven poses on the circle, visited in turn: consecutive controls always differ by a step or more)
            pose = synth.odometry_step(pose, 0.3, 0.9)
            odom = synth.odometry_step(odom, 0.3, 0.9)
        scan = synth.scan_points(synth.cast_scan(grid.cells, grid.resolution, origin, pose, angles, 8.0, 0.01, seed=c), angles)
        inputs.append((se2_from_xytheta(*odom), np.ascontiguousarray(scan)))
    # (the batch's inputs as the C call takes them, assembled outside the timed part: both ways are then one thin wrapper per C call)
    offsets = np.arange(n + 1, dtype=np.uint64) * BEAMS
    packed = [(np.tile(control, (n, 1)), np.tile(scan, (n, 1))) for control, scan in inputs]
    t0 = time.perf_counter()
    if by_batch:
        for controls, points in packed:
            if fleet.update_offsets(controls, points, offsets) != 0:
                raise RuntimeError("mcl_batch_update failed")
    else:
        for control, scan in inputs:
            for member in fleet.members:
                member.update(control, scan)
    return (time.perf_counter() - t0) / cycles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fleets", default="1,4,16,64,256")
    ap.add_argument("--cycles", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    cells = synth.make_rooms_map(128, 128, seed=3, n_rooms=6)
    grid = OccupancyGrid(cells=cells, resolution=0.05, origin=se2_from_xytheta(-3.2, -3.2, 0.0))
    start = synth.find_free_pose(cells, 0.05, (-3.2, -3.2), seed=3, clearance_cells=8)
    rows = []
    for members in [int(v) for v in args.fleets.split(",")]:
        for name, lo, hi in (("fixed 2000", 2000, 2000), ("KLD 500..2000", 500, 2000)):
            fleet = make_fleet(grid, members, lo, hi)
            for member in fleet.members:
                member.initialize(start, np.diag([0.04, 0.04, 0.01]))
            times = {True: [], False: []}
            cycle = 0
            for r in range(args.rounds + 1):
                for by_batch in (True, False):
                    t = drive(fleet, grid, start, args.cycles, cycle, by_batch)
                    cycle += args.cycles
                    if r:  # (round 0 is the untimed one)
                        times[by_batch].append(t)
            row = {"members": members, "fleet": name, "fused_share": fleet.counter("members_fused") / max(1, fleet.counter("members_fused") + fleet.counter("members_alone"))}
            for by_batch, key in ((True, "batch"), (False, "loop")):
                ms = np.array(times[by_batch]) * 1e3
                row[key] = {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
                            "per_filter_us": float(np.median(ms)) * 1e3 / members}
            row["ratio"] = row["batch"]["median_ms"] / row["loop"]["median_ms"]
            rows.append(row)
            print(f"F={members:4d} {name:14s} batch {row['batch']['median_ms']:8.4f} ms [{row['batch']['min_ms']:.4f}, {row['batch']['max_ms']:.4f}]"
                  f" = {row['batch']['per_filter_us']:7.2f} us/filter | loop {row['loop']['median_ms']:8.4f} ms [{row['loop']['min_ms']:.4f}, "
                  f"{row['loop']['max_ms']:.4f}] = {row['loop']['per_filter_us']:7.2f} us/filter | batch : loop {row['ratio']:.3f}"
                  f" | fused {row['fused_share']:.2f}", flush=True)
            fleet.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
