"""mcl_likelihoods against the only way to get the same numbers without it: a spare context of n particles with a second copy of the
map, mcl_set_particles + mcl_reweight + mcl_get_particles.

Shapes: n in {2000, 1e5, 1e6} poses spread over the turtlebot map x 180 and 1080 beams (likelihood-field model), and the NDT model on
the turtlebot NDT map with the measurement cells of a 360-beam scan of 3.5 m range (K is recorded: 14 cells with the committed map and
this scan - the 44 of the synthetic 200 m map's benchmark shape are not reached on the turtlebot world).  Both ways run in ONE
process, in alternating rounds - likelihoods, spare, likelihoods, spare, ... - after a warm-up of both; a figure is the median over
the rounds of the mean of `repeats` calls, host time around calls that end with the stream idle.  Writes profiles/likelihoods.json.

    python tools/exp_likelihoods.py [--rounds 5] [--repeats 5] [--out profiles/likelihoods.json]
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
from beluga_amd.amcl import (Amcl, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam, NDTModelParam2d, OccupancyGrid,  # noqa: E402
                             load_ndt_map_npz, se2_from_xytheta)

MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
SIZES = (2000, 100_000, 1_000_000)


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


def measure(make, measurement, poses, rounds, repeats):
    n = len(poses)
    running = make(2000)                 # the filter that is asked: its own set is small and stays untouched
    spare = make(n)                      # the spare context: a second map, a set of n
    ones = np.ones(n)

    def by_call():
        return running.likelihoods(poses, measurement)

    def by_spare():
        spare.set_particles(poses, ones)
        spare.reweight(measurement)
        return spare.particles()[1]

    a, b = by_call(), by_spare()  # (warm-up of both, and the two ways give the same numbers)
    worst = float(np.max(np.abs(a - b) / np.abs(b)))
    ms = {"likelihoods": [], "spare_context": []}
    for _ in range(rounds):
        ms["likelihoods"].append(timed(by_call, repeats))
        ms["spare_context"].append(timed(by_spare, repeats))
    running.close()
    spare.close()
    return {"n": n, "likelihoods_ms": statistics.median(ms["likelihoods"]), "spare_context_ms": statistics.median(ms["spare_context"]),
            "likelihoods_ms_rounds": ms["likelihoods"], "spare_context_ms_rounds": ms["spare_context"], "max_relative_difference": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "likelihoods.json"))
    args = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "turtlebot3_world_grid.npz"))
    cells, res = z["cells"], float(z["resolution"])
    ox, oy, ot = z["origin_xytheta"]
    grid = OccupancyGrid(cells=cells, resolution=res, origin=se2_from_xytheta(ox, oy, ot))
    truth = synth.find_free_pose(cells, res, (ox, oy), seed=4, clearance_cells=10)
    lf = LikelihoodFieldModelParam(2.0, 100.0, 0.5, 0.5, 0.2, True)
    ndt_map = load_ndt_map_npz(os.path.join(ROOT, "tests", "golden", "turtlebot3_world_ndt.npz"))
    results = []
    for beams in (180, 1080):
        angles = synth.lidar_angles(beams, 360.0)
        pts = synth.scan_points(synth.cast_scan(cells, res, (ox, oy), truth, angles, 3.5, 0.01, seed=1), angles)
        for n in SIZES:
            make = lambda cap: Amcl(grid, MOTION, lf, AmclParams(min_particles=cap, max_particles=cap), seed=3)
            r = measure(make, pts, spread_poses(cells, res, (ox, oy), n, 7), args.rounds, args.repeats)
            r.update(model="likelihood_field", beams=beams)
            results.append(r)
            print(json.dumps(r), flush=True)
    angles = synth.lidar_angles(360, 360.0)
    pts = synth.scan_points(synth.cast_scan(cells, res, (ox, oy), truth, angles, 3.5, 0.01, seed=1), angles)
    from beluga_amd.amcl import ndt_measurement_cells
    cells_k = len(ndt_measurement_cells(pts, ndt_map.resolution)[0])
    for n in SIZES:
        make = lambda cap: Amcl(ndt_map, MOTION, NDTModelParam2d(minimum_likelihood=0.01, d1=1.0, d2=0.6), AmclParams(min_particles=cap, max_particles=cap), seed=3)
        r = measure(make, pts, spread_poses(cells, res, (ox, oy), n, 7), args.rounds, args.repeats)
        r.update(model="ndt", beams=360, measurement_cells=cells_k)
        results.append(r)
        print(json.dumps(r), flush=True)
    record = {"what": "mcl_likelihoods vs a spare context (mcl_set_particles + mcl_reweight + mcl_get_particles), host ms per call, one process, "
                      "alternating rounds; median over the rounds of the mean of `repeats` calls", "rounds": args.rounds, "repeats": args.repeats,
              "map": "tests/golden/turtlebot3_world_grid.npz / turtlebot3_world_ndt.npz", "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
