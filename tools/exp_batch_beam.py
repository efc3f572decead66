"""Fleets of beam-model filters through mcl_batch_update: the members on the shared launches (option batch_beam_fused = 1) against
the members each running its own cycle inside the call (DESIGN.md "Batched small filters").

    python tools/exp_batch_beam.py [--fleets 1,8,64,256] [--cycles 40] [--rounds 7] [--json out.json]

Per fleet size F: F beam-model filters of 2000 particles x 180 beams, fixed size, on the turtlebot map (tests/golden).  Both settings of
the option alternate in one process on the same inputs: a timed round is `cycles` fleet updates with batch_beam_fused = 1 on every
member, then `cycles` with 0.  One untimed round, then `rounds` timed ones; reported: wall time per fleet update (median, minimum,
maximum over the rounds; the call ends behind its own synchronisation), the per-filter quotient, the ratio and the share of member
updates that went through the shared launches.

On a tree whose library does not know the option (the commit before it) the tool measures what such a tree does - every beam member
alone - under the name "alone": run there from a copy of this file, this is the comparison the option's gain is stated against; option 0
on a tree that has it is a cross-check of that number."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from beluga_amd import capi, synth  # noqa: E402
from beluga_amd.amcl import (AmclBatch, AmclParams, BeamModelParam, DifferentialDriveModelParam, OccupancyGrid,  # noqa: E402
                             se2_from_xytheta)

MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
BEAM = BeamModelParam(beam_max_range=12.0)
BEAMS = 180
PARTICLES = 2000


def turtlebot_grid(path):
    z = np.load(path)
    ox, oy, ot = z["origin_xytheta"]
    return OccupancyGrid(cells=z["cells"], resolution=float(z["resolution"]), origin=se2_from_xytheta(ox, oy, ot))


def make_inputs(grid, start, cycles, first_cycle, members):
    """The C call's inputs for `cycles` fleet updates (the robot visits seven poses on a circle in turn: every update moves)."""
    origin = (grid.origin[2], grid.origin[3])
    angles = synth.lidar_angles(BEAMS, 270.0)
    packed = []
    for c in range(first_cycle, first_cycle + cycles):
        pose, odom = start, (0.0, 0.0, 0.0)
        for _ in range(c % 7 + 1):
            pose = synth.odometry_step(pose, 0.15, 0.9)
            odom = synth.odometry_step(odom, 0.15, 0.9)
        scan = synth.scan_points(synth.cast_scan(grid.cells, grid.resolution, origin, pose, angles, 8.0, 0.01, seed=c), angles)
        packed.append((np.tile(se2_from_xytheta(*odom), (members, 1)), np.tile(np.ascontiguousarray(scan), (members, 1))))
    return packed


def drive(fleet, packed):
    """Seconds per fleet update (inputs assembled outside the timed part; mcl_batch_update returns behind its synchronisation)."""
    offsets = np.arange(len(fleet) + 1, dtype=np.uint64) * BEAMS
    t0 = time.perf_counter()
    for controls, points in packed:
        if fleet.update_offsets(controls, points, offsets) != 0:
            raise RuntimeError("mcl_batch_update failed")
    return (time.perf_counter() - t0) / len(packed)


def has_option(fleet):
    try:
        fleet.set_option("batch_beam_fused", 0)
        return True
    except capi.MclError:
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fleets", default="1,8,64,256")
    ap.add_argument("--cycles", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    ap.add_argument("--map", default=os.path.join(ROOT, "tests", "golden", "turtlebot3_world_grid.npz"))
    args = ap.parse_args()
    grid = turtlebot_grid(args.map)
    start = synth.find_free_pose(grid.cells, grid.resolution, (grid.origin[2], grid.origin[3]), seed=3, clearance_cells=6)
    rows = []
    for members in [int(v) for v in args.fleets.split(",")]:
        fleet = AmclBatch([dict(grid=grid, motion=MOTION, sensor=BEAM, params=AmclParams(min_particles=PARTICLES, max_particles=PARTICLES),
                                seed=1000 + i) for i in range(members)])
        for member in fleet.members:
            member.initialize(start, np.diag([0.04, 0.04, 0.01]))
        ways = ((1, "fused"), (0, "unfused")) if has_option(fleet) else ((None, "alone"),)
        times = {key: [] for _, key in ways}
        shared = {key: [0, 0] for _, key in ways}
        cycle = 0
        for r in range(args.rounds + 1):
            for value, key in ways:
                if value is not None:
                    fleet.set_option("batch_beam_fused", value)
                packed = make_inputs(grid, start, args.cycles, cycle, members)
                before = (fleet.counter("members_fused"), fleet.counter("members_alone"))
                t = drive(fleet, packed)
                cycle += args.cycles
                if r:  # (round 0 is the untimed one)
                    times[key].append(t)
                    shared[key][0] += fleet.counter("members_fused") - before[0]
                    shared[key][1] += fleet.counter("members_alone") - before[1]
        row = {"members": members, "fleet": f"beam model, fixed {PARTICLES} x {BEAMS}"}
        for _, key in ways:
            ms = np.array(times[key]) * 1e3
            row[key] = {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
                        "per_filter_us": float(np.median(ms)) * 1e3 / members,
                        "shared_share": shared[key][0] / max(1, shared[key][0] + shared[key][1])}
        text = f"F={members:4d}"
        for _, key in ways:
            v = row[key]
            text += (f" | {key} {v['median_ms']:8.4f} ms [{v['min_ms']:.4f}, {v['max_ms']:.4f}] = {v['per_filter_us']:7.2f} us/filter,"
                     f" shared {v['shared_share']:.2f}")
        if len(ways) == 2:
            row["ratio"] = row["fused"]["median_ms"] / row["unfused"]["median_ms"]
            row["fused_median_below_unfused_range"] = row["fused"]["median_ms"] < row["unfused"]["min_ms"]
            text += f" | fused : unfused {row['ratio']:.3f} | below the unfused range: {row['fused_median_below_unfused_range']}"
        rows.append(row)
        print(text, flush=True)
        fleet.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
