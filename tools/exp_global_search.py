"""One mcl_global_search call against the way the commit before it offers: the candidate poses enumerated on the host (numpy), scored with
mcl_likelihoods (host arrays) or mcl_likelihoods_device (torch tensors), the top `pool` taken by numpy / torch.

Shapes: the turtlebot map (tests/golden/turtlebot3_world_grid.npz) at stride 2, 72 headings with a 180-beam and a 1080-beam scan, and a
4096 x 4096 synthetic rooms map at stride 4, 72 headings, 180 beams.  All ways run in ONE process, in alternating rounds - search, host,
device, search, ... - after a warm-up of each; a figure is the median over the rounds of the host time of one call that ends with the
stream idle.  The enumeration on the host is timed apart from the scoring (a caller could keep it between scans of one map).  Every
way's pool is compared with the search's before anything is timed.  Writes profiles/global_search.json.

The split of a call's kernel time into generation, scoring and selection is not taken here (the call has no events of its own): run
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/exp_global_search.py --shapes tb3_180 --rounds 3 --out <file>
and add up k_search_select + k_search_generate, k_likelihoods_*, k_search_sort_tiles + k_search_merge_*; --kernels <stats csv> folds
such a file into the record under "kernel_split".

    python tools/exp_global_search.py [--rounds 5] [--shapes tb3_180,tb3_1080,synth4096] [--kernels stats.csv] [--out profiles/global_search.json]
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

from beluga_amd import synth  # noqa: E402
from beluga_amd.amcl import Amcl, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam, OccupancyGrid, se2_from_xytheta  # noqa: E402

MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
LF = LikelihoodFieldModelParam(max_obstacle_distance=2.0, max_laser_distance=100.0, z_hit=0.5, z_random=0.5, sigma_hit=0.2, model_unknown_space=True)
HEADINGS, POOL = 72, 1024


def turtlebot_grid():
    z = np.load(os.path.join(ROOT, "tests", "golden", "turtlebot3_world_grid.npz"))
    ox, oy, ot = z["origin_xytheta"]
    return OccupancyGrid(cells=z["cells"], resolution=float(z["resolution"]), origin=se2_from_xytheta(ox, oy, ot))


def synthetic_grid(size=4096):
    cells = synth.make_rooms_map(size, size, seed=42, n_rooms=130)
    return OccupancyGrid(cells=cells, resolution=0.05, origin=se2_from_xytheta(-size * 0.025, -size * 0.025, 0.0))


def scan_of(grid, beams, max_range):
    truth = synth.find_free_pose(grid.cells, grid.resolution, (grid.origin[2], grid.origin[3]), seed=2, clearance_cells=4)
    angles = synth.lidar_angles(beams, 270.0)
    return synth.scan_points(synth.cast_scan(grid.cells, grid.resolution, (grid.origin[2], grid.origin[3]), truth, angles, max_range, 0.01, 1), angles)


def enumerate_on_host(grid, stride, headings):
    """The header's rule in numpy: ids and poses (cos, sin, x, y) in id order."""
    H, W = grid.cells.shape
    free = np.flatnonzero(grid.cells.reshape(-1) == grid.value_traits[0])
    x, y = free % W, free // W
    cells = free[(x % stride == 0) & (y % stride == 0)]
    c, s, ox, oy = (float(v) for v in grid.origin)
    lx, ly = ((cells % W) + 0.5) * grid.resolution, ((cells // W) + 0.5) * grid.resolution
    gx, gy = (c * lx - s * ly) + ox, (s * lx + c * ly) + oy
    theta = -math.pi + np.arange(headings) * (2.0 * math.pi / headings)
    poses = np.empty((len(cells), headings, 4))
    poses[:, :, 0], poses[:, :, 1] = np.cos(theta)[None, :], np.sin(theta)[None, :]
    poses[:, :, 2], poses[:, :, 3] = gx[:, None], gy[:, None]
    ids = (cells.astype(np.uint64)[:, None] * np.uint64(headings) + np.arange(headings, dtype=np.uint64)[None, :]).reshape(-1)
    return ids, poses.reshape(-1, 4)


def top_on_host(ids, scores, pool):
    pool = min(pool, len(ids))
    part = np.argpartition(-scores, pool - 1)[:pool]
    cut = scores[part].min()
    among = np.flatnonzero(scores >= cut)  # ties at the cut: by id
    order = among[np.lexsort((ids[among], -scores[among]))]
    return ids[order[:pool]]


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def measure(name, grid, stride, beams, max_range, rounds):
    import torch

    f = Amcl(grid, MOTION, LF, AmclParams(max_particles=2000), seed=1)
    pts = scan_of(grid, beams, max_range)

    def by_search():
        return np.array([h.id for h in f.global_search_pool(pts, stride, HEADINGS, POOL)], dtype=np.uint64)

    def by_host(ids, poses):
        return top_on_host(ids, f.likelihoods(poses, pts), POOL)

    def by_device(ids_t, poses_t):
        scores = f.likelihoods_device(poses_t, pts)
        k = min(POOL, len(scores))
        cut = torch.topk(scores, k).values[-1]
        among = torch.nonzero(scores >= cut).reshape(-1)
        a_ids, a_scores = ids_t[among].cpu().numpy().astype(np.uint64), scores[among].cpu().numpy()
        return a_ids[np.lexsort((a_ids, -a_scores))][:k]

    t_enum, (ids, poses) = once(lambda: enumerate_on_host(grid, stride, HEADINGS))
    t_upload, (ids_t, poses_t) = once(lambda: (torch.from_numpy(ids.astype(np.int64)).cuda(), torch.from_numpy(poses).cuda()))
    torch.cuda.synchronize()
    # Warm-up, and the three ways give the same pool - up to candidates whose host-made rotation (numpy's cos / sin) differs in the last
    # bit from the table's, which can swap neighbours of almost equal score: the share of common ids is recorded, and has to be high.
    a, b, c = by_search(), by_host(ids, poses), by_device(ids_t, poses_t)
    common = (len(np.intersect1d(a, b)) / len(a), len(np.intersect1d(a, c)) / len(a))
    assert min(common) > 0.9, (name, common)
    info = dict(f.last_search_info)
    times = {"search": [], "host": [], "device": [], "enumerate": [t_enum]}
    for _ in range(rounds):
        times["search"].append(once(by_search)[0])
        times["host"].append(once(lambda: by_host(ids, poses))[0])
        times["device"].append(once(lambda: by_device(ids_t, poses_t))[0])
        times["enumerate"].append(once(lambda: enumerate_on_host(grid, stride, HEADINGS))[0])
    f.close()
    row = {"shape": name, "map": list(grid.cells.shape), "cell_stride": stride, "headings": HEADINGS, "pool": POOL, "beams": beams,
           "candidates": int(len(ids)), "pool_ids_in_common_with_host_and_device": list(common), "chunks": info["chunks"], "launches": info["launches"], "rounds": rounds,
           "global_search_ms": statistics.median(times["search"]), "global_search_ms_all": times["search"],
           "host_likelihoods_topk_ms": statistics.median(times["host"]), "host_likelihoods_topk_ms_all": times["host"],
           "device_likelihoods_topk_ms": statistics.median(times["device"]), "device_likelihoods_topk_ms_all": times["device"],
           "host_enumeration_ms": statistics.median(times["enumerate"]), "pose_upload_ms_once": t_upload}
    print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all")}), flush=True)
    return row


def kernel_split(path):
    """Sums a rocprofv3 kernel stats csv (columns Name, Calls, TotalDurationNs) into the call's three parts."""
    parts = {"generation_ns": 0, "scoring_ns": 0, "selection_ns": 0, "calls": {}}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name, total = r.get("Name", ""), int(float(r.get("TotalDurationNs", 0) or 0))
            key = ("generation_ns" if "k_search_select" in name or "k_search_generate" in name else
                   "scoring_ns" if "k_likelihoods" in name else
                   "selection_ns" if "k_search_sort_tiles" in name or "k_search_merge" in name else None)
            if key:
                parts[key] += total
                parts["calls"][name.split("(")[0]] = {"calls": int(r.get("Calls", 0) or 0), "total_ns": total}
    return parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="tb3_180,tb3_1080,synth4096")
    ap.add_argument("--kernels", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_search.json"))
    args = ap.parse_args()
    rows = []
    for shape in args.shapes.split(","):
        if shape == "tb3_180":
            rows.append(measure(shape, turtlebot_grid(), 2, 180, 3.5, args.rounds))
        elif shape == "tb3_1080":
            rows.append(measure(shape, turtlebot_grid(), 2, 1080, 3.5, args.rounds))
        elif shape == "synth4096":
            rows.append(measure(shape, synthetic_grid(), 4, 180, 12.0, max(2, args.rounds // 2)))
        else:
            raise SystemExit(f"unknown shape {shape}")
    record = {"what": "one mcl_global_search_pool call against host-enumerated poses through mcl_likelihoods / mcl_likelihoods_device and a host / torch "
                      "top-k; host milliseconds around calls that end with the stream idle, median over alternating rounds in one process",
              "rows": rows}
    if args.kernels:
        record["kernel_split"] = kernel_split(args.kernels)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
