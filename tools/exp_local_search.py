"""One mcl_local_search call against the way the commit before it offers: the lattice's poses enumerated on the host (numpy), scored with
mcl_likelihoods (host arrays), the best and the ten moments taken with numpy.

Shapes: the turtlebot map (tests/golden/turtlebot3_world_grid.npz) with 1 and 16 seeds, the default lattice (4, 5) and (8, 16), a 180-beam
and a 1080-beam scan; and the turtlebot NDT map (tests/golden/turtlebot3_world_ndt.npz) with 16 seeds and the default lattice.  Both
ways run in ONE process, in alternating rounds - search, host, search, ... - after a warm-up of each; a figure is the median over the
rounds of the host time of one call that ends with the stream idle.  The enumeration on the host and the upload of its poses (inside
mcl_likelihoods: timed as a torch copy of the same array) are listed apart from the host way's total.  Both ways' best candidates are
compared before anything is timed.  Also recorded: a scenario's distance to the truth before and after (the 64 x 48 map of
tests/test_gpu_local_search.py).  Writes profiles/local_search.json.

The split of a call's kernel time into generation, scoring and reduction is not taken here (the call has no events of its own): run
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/exp_local_search.py --shapes tb3_16_default_180 --rounds 3 --out <file>
and --kernels <stats csv> folds such a file into the record under "kernel_split".

    python tools/exp_local_search.py [--rounds 5] [--shapes all] [--kernels stats.csv] [--out profiles/local_search.json]
"""
import argparse
import csv
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import local_search_reference as ref  # noqa: E402
from beluga_amd import synth  # noqa: E402
from beluga_amd.amcl import (Amcl, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam, NDTModelParam2d, OccupancyGrid,  # noqa: E402
                             load_ndt_map_npz, se2_from_xytheta)

MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
LF = LikelihoodFieldModelParam(max_obstacle_distance=2.0, max_laser_distance=100.0, z_hit=0.5, z_random=0.5, sigma_hit=0.2, model_unknown_space=True)
STEP_THETA = math.pi / 360
SHAPES = {  # name: (map, seeds, (Kx, Kt), beams)
    "tb3_1_default_180": ("grid", 1, (4, 5), 180), "tb3_16_default_180": ("grid", 16, (4, 5), 180), "tb3_1_8x16_180": ("grid", 1, (8, 16), 180),
    "tb3_16_8x16_180": ("grid", 16, (8, 16), 180), "tb3_1_default_1080": ("grid", 1, (4, 5), 1080), "tb3_16_default_1080": ("grid", 16, (4, 5), 1080),
    "tb3_16_8x16_1080": ("grid", 16, (8, 16), 1080), "ndt_16_default_180": ("ndt", 16, (4, 5), 180),
}


def turtlebot_grid():
    z = np.load(os.path.join(ROOT, "tests", "golden", "turtlebot3_world_grid.npz"))
    ox, oy, ot = z["origin_xytheta"]
    return OccupancyGrid(cells=z["cells"], resolution=float(z["resolution"]), origin=se2_from_xytheta(ox, oy, ot))


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def enumerate_on_host(seeds, Kx, Kt, step_xy):
    return np.concatenate([ref.lattice_poses(s, Kx, Kt, step_xy, STEP_THETA) for s in seeds])


def best_and_moments_on_host(scores, n, Kx, Kt):
    """numpy's argmax (ties to the lowest id: NOT the search's tie rule, which costs more) and the ten moments, per seed."""
    L = ref.candidates(Kx, Kt)
    i, j, k = ref.offsets_of(Kx, Kt, np.arange(L))
    factors = np.stack([np.ones(L), i, j, k, i * i, i * j, i * k, j * j, j * k, k * k]).astype(np.float64)
    w = scores.reshape(n, L)
    return w.argmax(axis=1), w @ factors.T


def measure(name, rounds):
    import torch

    kind, n, (Kx, Kt), beams = SHAPES[name]
    grid = turtlebot_grid()
    truth = synth.find_free_pose(grid.cells, grid.resolution, (grid.origin[2], grid.origin[3]), seed=2, clearance_cells=4)
    angles = synth.lidar_angles(beams, 270.0)
    pts = synth.scan_points(synth.cast_scan(grid.cells, grid.resolution, (grid.origin[2], grid.origin[3]), truth, angles, 3.5, 0.01, 1), angles)
    if kind == "grid":
        f = Amcl(grid, MOTION, LF, AmclParams(max_particles=2000), seed=1)
        step_xy = 0.25 * grid.resolution
    else:
        ndt_map = load_ndt_map_npz(os.path.join(ROOT, "tests", "golden", "turtlebot3_world_ndt.npz"))
        f = Amcl(ndt_map, MOTION, NDTModelParam2d(), AmclParams(max_particles=2000), seed=1)
        step_xy = 0.25 * ndt_map.resolution
    rng = np.random.default_rng(6)
    seeds = np.array([se2_from_xytheta(truth[0] + rng.uniform(-0.05, 0.05), truth[1] + rng.uniform(-0.05, 0.05), truth[2] + rng.uniform(-0.04, 0.04))
                      for _ in range(n)])

    def by_search():
        return f.local_search(seeds, pts, Kx, Kt, None, STEP_THETA)

    def by_host():
        poses = enumerate_on_host(seeds, Kx, Kt, step_xy)
        return best_and_moments_on_host(f.likelihoods(poses, pts), n, Kx, Kt)

    hits, (best, sums) = by_search(), by_host()  # warm-up, and the two ways agree
    same_score = [float(h.score) == float(f.likelihoods(ref.lattice_poses(s, Kx, Kt, step_xy, STEP_THETA)[b][None, :], pts)[0]) for h, s, b in zip(hits, seeds, best)]
    assert all(same_score), name
    assert np.allclose(np.array([h.sums for h in hits]), sums, rtol=1e-9, atol=1e-9), name
    info = dict(f.last_local_search_info)
    poses = enumerate_on_host(seeds, Kx, Kt, step_xy)
    times = {"search": [], "host": [], "enumerate": [], "upload": []}
    for _ in range(rounds):
        times["search"].append(once(by_search)[0])
        times["host"].append(once(by_host)[0])
        times["enumerate"].append(once(lambda: enumerate_on_host(seeds, Kx, Kt, step_xy))[0])

        def upload():
            t = torch.from_numpy(poses).cuda()
            torch.cuda.synchronize()
            return t

        times["upload"].append(once(upload)[0])
    f.close()
    row = {"shape": name, "map": kind, "seeds": n, "half_steps": [Kx, Kt], "beams": beams, "candidates_per_seed": info["candidates_per_seed"],
           "passes": info["passes"], "launches": info["launches"], "rounds": rounds,
           "local_search_ms": statistics.median(times["search"]), "local_search_ms_all": times["search"],
           "host_enumerate_likelihoods_numpy_ms": statistics.median(times["host"]), "host_enumerate_likelihoods_numpy_ms_all": times["host"],
           "of_which_host_enumeration_ms": statistics.median(times["enumerate"]), "of_which_pose_upload_ms": statistics.median(times["upload"])}
    print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all")}), flush=True)
    return row


def scenario():
    """tests/test_gpu_local_search.py's scenario: the truth 0.03 m, -0.02 m and 2.3 degrees off a candidate of the global search."""
    W, H = 64, 48
    cells = np.zeros((H, W), dtype=np.int8)
    cells[0, :] = cells[-1, :] = cells[:, 0] = cells[:, -1] = 100
    cells[30, [x for x in range(W) if x < 12 or x > 18]] = 100
    cells[:30, 40] = 100
    grid = OccupancyGrid(cells=cells, resolution=0.1, origin=se2_from_xytheta(-1.0, -1.0, 0.0))
    f = Amcl(grid, MOTION, LF, AmclParams(max_particles=64), seed=1)
    truth = (0.05 + 0.03, 0.05 - 0.02, math.radians(2.3))
    angles = np.linspace(-math.pi, math.pi, 90, endpoint=False)
    ranges = f.expected_scan(truth, angles, max_range=8.0)
    pts = np.column_stack([ranges * np.cos(angles), ranges * np.sin(angles)])
    seed = f.global_search(pts)[0]
    h = f.local_search(seed.pose[None, :], pts)[0]
    f.close()

    def distance(pose):
        return {"metres": math.hypot(pose[2] - truth[0], pose[3] - truth[1]),
                "radians": abs(math.remainder(math.atan2(pose[1], pose[0]) - truth[2], 2 * math.pi))}

    return {"seed": distance(seed.pose), "best": distance(h.pose), "mean": distance(h.mean_pose), "offsets": [h.di, h.dj, h.dk], "plateau": h.plateau}


def kernel_split(path):
    """Sums a rocprofv3 kernel stats csv (columns Name, Calls, TotalDurationNs) into the call's three parts."""
    parts = {"generation_ns": 0, "scoring_ns": 0, "reduction_ns": 0, "calls": {}}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name, total = r.get("Name", ""), int(float(r.get("TotalDurationNs", 0) or 0))
            key = ("generation_ns" if "k_local_generate" in name else "scoring_ns" if "k_likelihoods" in name else
                   "reduction_ns" if "k_local_reduce" in name else None)
            if key:
                parts[key] += total
                parts["calls"][name.split("(")[0]] = {"calls": int(r.get("Calls", 0) or 0), "total_ns": total}
    return parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="all")
    ap.add_argument("--kernels", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_search.json"))
    args = ap.parse_args()
    names = list(SHAPES) if args.shapes == "all" else args.shapes.split(",")
    rows = [measure(name, args.rounds) for name in names]
    record = {"what": "one mcl_local_search call against host-enumerated lattice poses through mcl_likelihoods and numpy's argmax and moments; host "
                      "milliseconds around calls that end with the stream idle, median over alternating rounds in one process",
              "rows": rows, "scenario_distance_to_truth": scenario()}
    if args.kernels:
        record["kernel_split"] = kernel_split(args.kernels)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
