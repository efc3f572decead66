"""Fleets of small filters: mcl_batch_update against a loop of mcl_update over the same members (DESIGN.md "Batched small filters").

    python tools/exp_batch.py [--fleets 1,4,16,64,256] [--cycles 40] [--rounds 7] [--json out.json] [--estimate cluster]

Per fleet size F, two fleets on one small map: F filters of 2000 particles x 180 beams, fixed size, and the same KLD-adaptive
(500 .. 2000).  Both ways of updating alternate in one process on the same inputs: a timed round is `cycles` fleet updates through
mcl_batch_update, then `cycles` fleet updates by a loop of mcl_update over the members (the members are ordinary contexts, so the loop
is what a caller without the batch does).  One untimed round, then `rounds` timed ones; reported: wall time per fleet update (median,
minimum, maximum over the rounds), the per-filter quotient and the ratio batch : loop.

--estimate cluster: every member returns the cluster-based estimate (estimate_kind = 1, what the ROS facade returns), fixed 2000
particles, and the two ways that alternate are both mcl_batch_update: the members' option batch_cluster_fused = 1 (two shared launches for the fleet's
estimates) against batch_cluster_fused = 0 (every member's own mcl_cluster_based_estimate).  Reported per fleet size: median and range of both,
whether the fused median lies below the unfused range (the rule the default goes by at F = 16 and F = 64), and the share of the fused
time that the host spends between the two launches, one member after the other (counter cluster_host_ns: cells ordered, assign_clusters,
cluster ids written)."""
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


def cluster_mode(args, grid, start):
    rows = []
    for members in [int(v) for v in args.fleets.split(",")]:
        fleet = make_fleet(grid, members, 2000, 2000)
        for member in fleet.members:
            member.set_estimate_kind(cluster_based=True)
            member.initialize(start, np.diag([0.04, 0.04, 0.01]))
        times, host_share = {1: [], 0: []}, []
        cycle = 0
        for r in range(args.rounds + 1):
            for fused in (1, 0):
                fleet.set_option("batch_cluster_fused", fused)
                host0 = fleet.counter("cluster_host_ns")
                t = drive(fleet, grid, start, args.cycles, cycle, True)
                cycle += args.cycles
                if r:  # (round 0 is the untimed one)
                    times[fused].append(t)
                    if fused:
                        host_share.append((fleet.counter("cluster_host_ns") - host0) * 1e-9 / args.cycles / t)
        row = {"members": members, "fleet": "fixed 2000, cluster-based estimate"}
        for fused, key in ((1, "fused"), (0, "unfused")):
            ms = np.array(times[fused]) * 1e3
            row[key] = {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
                        "per_filter_us": float(np.median(ms)) * 1e3 / members}
        row["ratio"] = row["fused"]["median_ms"] / row["unfused"]["median_ms"]
        row["fused_median_below_unfused_range"] = row["fused"]["median_ms"] < row["unfused"]["min_ms"]
        row["host_share_of_fused"] = float(np.median(host_share))
        rows.append(row)
        print(f"F={members:4d} fused {row['fused']['median_ms']:8.4f} ms [{row['fused']['min_ms']:.4f}, {row['fused']['max_ms']:.4f}]"
              f" = {row['fused']['per_filter_us']:7.2f} us/filter | unfused {row['unfused']['median_ms']:8.4f} ms "
              f"[{row['unfused']['min_ms']:.4f}, {row['unfused']['max_ms']:.4f}] = {row['unfused']['per_filter_us']:7.2f} us/filter | "
              f"fused : unfused {row['ratio']:.3f} | below the unfused range: {row['fused_median_below_unfused_range']} | "
              f"host pass {100 * row['host_share_of_fused']:.1f} % of fused", flush=True)
        fleet.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fleets", default="1,4,16,64,256")
    ap.add_argument("--cycles", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    ap.add_argument("--estimate", default="mean", choices=["mean", "cluster"])
    args = ap.parse_args()
    cells = synth.make_rooms_map(128, 128, seed=3, n_rooms=6)
    grid = OccupancyGrid(cells=cells, resolution=0.05, origin=se2_from_xytheta(-3.2, -3.2, 0.0))
    start = synth.find_free_pose(cells, 0.05, (-3.2, -3.2), seed=3, clearance_cells=8)
    if args.estimate == "cluster":
        rows = cluster_mode(args, grid, start)
    else:
        rows = mean_mode(args, grid, start)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


def mean_mode(args, grid, start):
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
    return rows


if __name__ == "__main__":
    main()
