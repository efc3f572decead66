"""mcl_cast_rays timed: host time per call with the stream idle at the end, in alternating rounds in one process.

Shapes (poses x bearings): 1 x 360, 2000 x 180, 100 000 x 360, 1 000 000 x 60, poses spread over the map.  Maps: the turtlebot map
(max_range 3.5 m) and a synthetic 4096 x 4096 rooms map (max_range 30 m).  Contexts: a beam context (the packed bit maps) and a
likelihood-field context (the int8 cells).  Per shape, map and context: the host form (poses up, ranges and hit cells down: the copies are
in the figure) and the device form over torch tensors (no copies: the kernels and their launches), rays/s and cells visited per second
of each.  Yardsticks beside them: mcl_likelihoods on the beam context at the same poses with scan points along the same bearings (the same
walk plus the mixture, a wave per pose; its device form) and, at 1 x 360, the CPU oracle's ray_cast in a loop - the only way without this
entry point.  A figure is the median over the rounds of the mean of `repeats` calls.  Writes profiles/cast_rays.json.

    python tools/exp_cast_rays.py [--rounds 3] [--repeats 3] [--out profiles/cast_rays.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from beluga_amd import synth  # noqa: E402
from beluga_amd.amcl import (Amcl, AmclParams, BeamModelParam, DifferentialDriveModelParam, LikelihoodFieldModelParam, OccupancyGrid,  # noqa: E402
                             se2_from_xytheta)

MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
SHAPES = ((1, 360), (2000, 180), (100_000, 360), (1_000_000, 60))


def spread_poses(cells, res, origin, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    H, W = cells.shape
    theta = rng.uniform(-np.pi, np.pi, n)
    return np.ascontiguousarray(np.stack([np.cos(theta), np.sin(theta), origin[0] + rng.uniform(0, W * res, n), origin[1] + rng.uniform(0, H * res, n)], axis=1))


def timed(fn, repeats):
    t0 = time.perf_counter()
    for _ in range(repeats):
        fn()
    return (time.perf_counter() - t0) / repeats * 1e3


def measure(name, grid, max_range, rounds, repeats, oracle):
    import torch

    cells, res, origin = grid.cells, grid.resolution, (grid.origin[2], grid.origin[3])
    beam = Amcl(grid, MOTION, BeamModelParam(0.5, 0.05, 0.05, 0.5, 0.2, 0.1, max_range), AmclParams(min_particles=100, max_particles=100), seed=3)
    lf = Amcl(grid, MOTION, LikelihoodFieldModelParam(2.0, 100.0, 0.5, 0.5, 0.2, True), AmclParams(min_particles=100, max_particles=100), seed=3)
    results = []
    for n, B in SHAPES:
        poses = spread_poses(cells, res, origin, n, 7)
        angles = 2 * np.pi * np.arange(B) / B
        d_poses = torch.from_numpy(poses).to("cuda:0")
        points = 0.5 * max_range * np.stack([np.cos(angles), np.sin(angles)], axis=1)
        ways = {}
        for kind, f in (("beam_bits", beam), ("lf_cells", lf)):
            ways[kind + "_host"] = lambda f=f: f.cast_rays(poses, angles=angles, max_range=max_range, hit_cells=True)
            ways[kind + "_device"] = lambda f=f: f.cast_rays_device(d_poses, angles=angles, max_range=max_range, hit_cells=True)
        ways["likelihoods_beam_device"] = lambda: beam.likelihoods_device(d_poses, points)
        _, _, cells_visited = beam.cast_rays(poses, angles=angles, max_range=max_range, hit_cells=True, cells_visited=True)
        a = beam.cast_rays(poses, angles=angles, max_range=max_range)
        assert np.array_equal(a, lf.cast_rays(poses, angles=angles, max_range=max_range))  # (and a warm-up of both)
        for fn in ways.values():
            fn()
        ms = {k: [] for k in ways}
        for _ in range(rounds):
            for k, fn in ways.items():
                ms[k].append(timed(fn, repeats))
        r = {"map": name, "poses": n, "bearings": B, "rays": n * B, "max_range": max_range, "cells_visited": cells_visited,
             "hit_fraction": float((a < max_range).mean())}
        for k, v in ms.items():
            med = statistics.median(v)
            r[k + "_ms"] = med
            r[k + "_ms_rounds"] = v
            r[k + "_rays_per_s"] = n * B / (med * 1e-3)
            if k != "likelihoods_beam_device":
                r[k + "_cells_per_s"] = cells_visited / (med * 1e-3)
        if oracle and n == 1:
            from oracle import binding as orc
            t0 = time.perf_counter()
            for a_ in angles:
                orc.ray_cast(cells, res, grid.origin, poses[0], max_range, float(a_))
            r["oracle_cpu_loop_ms"] = (time.perf_counter() - t0) * 1e3
        results.append(r)
        print(json.dumps(r), flush=True)
        del d_poses
    beam.close()
    lf.close()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cast_rays.json"))
    args = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "turtlebot3_world_grid.npz"))
    ox, oy, ot = z["origin_xytheta"]
    turtlebot = OccupancyGrid(cells=z["cells"], resolution=float(z["resolution"]), origin=se2_from_xytheta(ox, oy, ot))
    big = OccupancyGrid(cells=synth.make_rooms_map(4096, 4096, seed=42), resolution=0.05, origin=se2_from_xytheta(-102.4, -102.4, 0.0))
    results = measure("turtlebot3_world", turtlebot, 3.5, args.rounds, args.repeats, not args.no_oracle)
    results += measure("synthetic_4096x4096", big, 30.0, args.rounds, args.repeats, not args.no_oracle)
    record = {"what": "mcl_cast_rays: host ms per call, stream idle at the end, one process, alternating rounds; median over the rounds of the mean of "
                      "`repeats` calls.  *_host: poses up, ranges and hit cells down (copies included); *_device: torch tensors, no copies; "
                      "likelihoods_beam_device: mcl_likelihoods_device on the beam context, scan points along the same bearings (the same walk plus "
                      "the mixture); oracle_cpu_loop_ms: the CPU oracle's ray_cast, one call per ray",
              "rounds": args.rounds, "repeats": args.repeats, "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
