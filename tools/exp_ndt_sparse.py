"""The hashed layout of the NDT map (mcl_set_ndt_map_layout 2) against the dense one (0) on maps BOTH hold, in one process.

Three cases, each with two filters on the same map and seed, one per layout, measured in alternating blocks (dense, hashed, dense,
hashed, ...) so that a drift of the machine shows in both: the synthetic 200 m map at 1M particles x 1080 beams, and the turtlebot NDT
map at config 1 (KLD 500 .. 2000 particles, 360 beams) with the small cycle off and on.  Per block: `cycles` timed update cycles with
profiling off (cycles/s of the whole update as the Python caller sees it), then `cycles` more with HIP events around the sensor kernel
(profile level 1: its mean time; with profiling on a small set takes the ordinary cycle, but the reweight kernel is the same one).  20
warm-up cycles per filter first.  Reports each figure as median and range over the blocks, the map's device bytes in each layout
(index structure + records + keys, from the layouts' definitions), and whether the two filters' particle sets ended bit-identical.
Writes profiles/ndt_sparse_map.json.

    python tools/exp_ndt_sparse.py [--repeats 5] [--cycles 50]
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
from beluga_amd.amcl import (Amcl, AmclParams, DifferentialDriveModelParam, NDTMap2d, NDTModelParam2d, load_ndt_map_npz,  # noqa: E402
                             ndt_measurement_cells, se2_from_xytheta)

NODE = NDTModelParam2d(minimum_likelihood=0.01, d1=1.0, d2=0.6)
WARMUP = 20
LAYOUTS = (("dense", 0), ("hashed", 2))


def map_bytes(m, reach=1):
    """Device bytes of the map in each layout: the int32 index grid over the keys' box with its border of 2 x reach, or the table of
    16-byte slots (the smallest power of two >= 2 x cells), plus what both hold: 48-byte records and the keys."""
    keys = np.asarray(m.cells, dtype=np.int64).reshape(-1, 2)
    n = len(keys)
    w, h = (int(keys[:, a].max() - keys[:, a].min()) + 1 + 4 * reach for a in (0, 1))
    slots = 2
    while slots < 2 * n:
        slots *= 2
    shared = n * (48 + 8)
    return {"cells": n, "dense": {"index_grid": 4 * w * h, "total": 4 * w * h + shared}, "hashed": {"table": 16 * slots, "total": 16 * slots + shared}}


def spread(values, digits):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits)}


def run(name, m, cells, res, origin, n_min, n_max, beams, max_range, small, repeats, cycles):
    truth = synth.find_free_pose(cells, res, origin, seed=4, clearance_cells=10)
    angles = synth.lidar_angles(beams, 360.0)
    pts = synth.scan_points(synth.cast_scan(cells, res, origin, truth, angles, max_range, 0.01, seed=1), angles)
    filters, poses = {}, {}
    for layout, mode in LAYOUTS:
        f = Amcl(m, DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05), NODE, AmclParams(min_particles=n_min, max_particles=n_max), seed=3,
                 ndt_small_cycle=small, ndt_map_layout=mode)
        assert f.ndt_map_layout() == (mode, 1 if mode else 0)
        f.initialize(truth, np.diag([0.04, 0.04, 0.01]))
        filters[layout], poses[layout] = f, np.array(truth, dtype=np.float64)

    def cycle(layout, c):
        poses[layout] = poses[layout] + np.array([0.0, 0.0, 0.001 if c % 2 else -0.001])
        filters[layout].force_update()
        filters[layout].update(se2_from_xytheta(*poses[layout]), pts)

    for layout, _ in LAYOUTS:
        for c in range(WARMUP):
            cycle(layout, c)
    rates = {layout: [] for layout, _ in LAYOUTS}
    kernel_ms = {layout: [] for layout, _ in LAYOUTS}
    for _ in range(repeats):
        for layout, _ in LAYOUTS:  # (alternating: dense, hashed, dense, hashed, ...)
            f = filters[layout]
            t0 = time.perf_counter()
            for c in range(cycles):
                cycle(layout, c)
            rates[layout].append(cycles / (time.perf_counter() - t0))
            f.profile_enable(1)
            f.profile_read(reset=True)
            for c in range(cycles):
                cycle(layout, c)
            ms, cnt = f.profile_read(reset=True)["sensor_kernel"]
            f.profile_enable(0)
            kernel_ms[layout].append(ms / cnt if cnt else float("nan"))
    (s0, w0), (s1, w1) = filters["dense"].particles(), filters["hashed"].particles()
    out = {"case": name, "small_cycle": bool(small), "particles": filters["dense"].num_particles(), "beams": beams,
           "K": int(len(ndt_measurement_cells(pts, m.resolution)[0])), "map_bytes": map_bytes(m),
           "sets_bit_identical": bool(np.array_equal(s0.view(np.uint64), s1.view(np.uint64)) and np.array_equal(w0.view(np.uint64), w1.view(np.uint64)))}
    for layout, _ in LAYOUTS:
        out[layout] = {"cycles_per_s": spread(rates[layout], 2), "sensor_kernel_ms": spread(kernel_ms[layout], 4)}
    ratios = [h / d for h, d in zip(rates["hashed"], rates["dense"])]  # block by block: neighbours in time
    out["cycles_per_s_hashed_over_dense"] = spread(ratios, 3)
    out["sensor_kernel_hashed_over_dense"] = spread([h / d for h, d in zip(kernel_ms["hashed"], kernel_ms["dense"])], 3)
    for f in filters.values():
        f.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ndt_sparse_map.json"))
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "turtlebot3_world_grid.npz"))
    tb = load_ndt_map_npz(os.path.join(ROOT, "tests", "golden", "turtlebot3_world_ndt.npz"))
    tb_args = (tb, z["cells"], float(z["resolution"]), tuple(z["origin_xytheta"][:2]), 500, 2000, 360, 3.5)
    results = [run("config1_turtlebot", *tb_args, False, a.repeats, a.cycles), run("config1_turtlebot_small_cycle", *tb_args, True, a.repeats, a.cycles)]
    cells = synth.make_rooms_map(4000, 4000, seed=42)
    keys, means, covs = synth.make_ndt_map(cells, 0.05, 1.0, origin_xy=(-100.0, -100.0), seed=1)
    results.append(run("synthetic_200m_1M", NDTMap2d(keys, means, covs, 1.0), cells, 0.05, (-100.0, -100.0), 1_000_000, 1_000_000, 1080, 30.0,
                       False, a.repeats, a.cycles))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"warmup_cycles": WARMUP, "repeats": a.repeats, "cycles": a.cycles, "cases": results}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
