"""A fleet on one map: every member uploads its own (mcl_set_map per member) against one shared map and F attaches (DESIGN.md "Shared maps").

    python tools/exp_shared_map.py [--fleets 16,64] [--size 2048] [--cycles 20] [--rounds 5] [--out profiles/shared_map.txt]

Per fleet size F: F filters of 2000 particles x 180 beams in one AmclBatch on one size x size map.  Both variants run in ONE process, one
after the other: the members' own mcl_set_map, then mcl_shared_map_create once and mcl_use_shared_map F times.  Recorded per variant: the
set-up's wall time, the drop in free device memory across it (hipMemGetInfo through torch), and the fleet update time - `rounds` timed
rounds of `cycles` mcl_batch_update each after one untimed round, median and range.  Records, not gates."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from beluga_amd import synth  # noqa: E402
from beluga_amd.amcl import (AmclBatch, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam, OccupancyGrid,  # noqa: E402
                             SharedMap, se2_from_xytheta)

MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
LF = LikelihoodFieldModelParam(2.0, 100.0, 0.5, 0.5, 0.2, True)
BEAMS = 180
COV = np.diag([0.04, 0.04, 0.01])


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def inputs_for(grid, start, cycles, members):
    origin = (grid.origin[2], grid.origin[3])
    angles = synth.lidar_angles(BEAMS, 270.0)
    out = []
    for c in range(cycles):
        pose, odom = start, (0.0, 0.0, 0.0)
        for _ in range(c % 7 + 1):  # (seven poses on a circle, visited in turn: consecutive controls always differ by a step or more)
            pose = synth.odometry_step(pose, 0.3, 0.9)
            odom = synth.odometry_step(odom, 0.3, 0.9)
        scan = synth.scan_points(synth.cast_scan(grid.cells, grid.resolution, origin, pose, angles, 8.0, 0.01, seed=c), angles)
        out.append((np.tile(se2_from_xytheta(*odom), (members, 1)), np.tile(np.ascontiguousarray(scan), (members, 1))))
    return out


def timed_rounds(fleet, inputs, rounds):
    offsets = np.arange(len(fleet) + 1, dtype=np.uint64) * BEAMS
    per_update = []
    for r in range(rounds + 1):
        t0 = time.perf_counter()
        for controls, points in inputs:
            fleet.update_offsets(controls, points, offsets)
        if r:  # (the first round is untimed)
            per_update.append((time.perf_counter() - t0) / len(inputs))
    return np.array(per_update) * 1e3


def variant(grid, start, members, shared, inputs, rounds):
    specs = [dict(grid=None, motion=MOTION, sensor=LF, params=AmclParams(min_particles=2000, max_particles=2000), seed=1000 + i)
             for i in range(members)]
    fleet = AmclBatch(specs)
    before = free_bytes()
    t0 = time.perf_counter()
    handle = None
    if shared:
        handle = SharedMap(grid, LF)
        for member in fleet.members:
            member.use_map(handle)
    else:
        for member in fleet.members:
            member.update_map(grid)
    setup_s = time.perf_counter() - t0
    used = before - free_bytes()
    for member in fleet.members:
        member.initialize(start, COV)
    ms = timed_rounds(fleet, inputs, rounds)
    fused = fleet.counter("members_fused")
    fleet.close()
    if handle is not None:
        handle.close()
    return dict(setup_s=setup_s, device_mb=used / 2**20, median=float(np.median(ms)), lo=float(ms.min()), hi=float(ms.max()), fused=fused)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fleets", default="16,64")
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cells = synth.make_rooms_map(args.size, args.size, seed=42, n_rooms=max(3, args.size * args.size // 120000))
    grid = OccupancyGrid(cells=cells, resolution=0.05, origin=se2_from_xytheta(0.0, 0.0, 0.0))
    start = synth.find_free_pose(cells, grid.resolution, (0.0, 0.0), seed=3, clearance_cells=10)
    lines = [f"# {args.size} x {args.size} map, members of 2000 particles x {BEAMS} beams, {args.rounds} rounds of {args.cycles} fleet updates",
             "# F variant      set-up s   device MB   update ms median (min .. max)   members fused"]
    for members in [int(v) for v in args.fleets.split(",")]:
        inputs = inputs_for(grid, start, args.cycles, members)
        for shared in (False, True):
            r = variant(grid, start, members, shared, inputs, args.rounds)
            lines.append(f"{members:4d} {'shared ' if shared else 'private'}  {r['setup_s']:10.3f}  {r['device_mb']:10.1f}   "
                         f"{r['median']:.3f} ({r['lo']:.3f} .. {r['hi']:.3f})   {r['fused']}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
