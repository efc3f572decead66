"""NDT sensor model: cycles/s of the whole update and the NDT kernel's time (HIP events around the sensor kernel, profile level 1),
at 1M particles x 1080 beams on the synthetic 200 m map (4000^2 cells at 5 cm, NDT cells of 1 m), and at config-1 sizes (KLD
500 .. 2000 particles, 360 beams) on the turtlebot NDT map.  Also reports K (measurement cells per scan) and the mean number of
map cells present per look-up (kernel offsets that find a cell), from the restatement on a sample of particles.

    python tools/exp_ndt.py [--repeats 5] [--cycles 50]
"""
import argparse
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
from beluga_amd.amcl import (Amcl, AmclParams, DifferentialDriveModelParam, NDTMap2d, NDTModelParam2d, load_ndt_map_npz,  # noqa: E402
                             ndt_measurement_cells, se2_from_xytheta)

NODE = NDTModelParam2d(minimum_likelihood=0.01, d1=1.0, d2=0.6)
KERNEL = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 0), (0, 1), (1, -1), (1, 0), (1, 1))


def present_per_lookup(m, states, means):
    keys = {tuple(k) for k in np.asarray(m.cells)}
    hits = looks = 0
    for st in states:
        c, s, x, y = st
        for mu in means:
            ux, uy = c * mu[0] - s * mu[1] + x, s * mu[0] + c * mu[1] + y
            cx, cy = math.floor(ux / m.resolution), math.floor(uy / m.resolution)
            looks += 1
            hits += sum((cx + dx, cy + dy) in keys for dx, dy in KERNEL)
    return hits / max(looks, 1)


def run(name, m, cells, res, origin, n_min, n_max, beams, max_range, repeats, cycles):
    truth = synth.find_free_pose(cells, res, origin, seed=4, clearance_cells=10)
    f = Amcl(m, DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05), NODE, AmclParams(min_particles=n_min, max_particles=n_max), seed=3)
    f.initialize(truth, np.diag([0.04, 0.04, 0.01]))
    angles = synth.lidar_angles(beams, 360.0)
    pts = synth.scan_points(synth.cast_scan(cells, res, origin, truth, angles, max_range, 0.01, seed=1), angles)
    means, _ = ndt_measurement_cells(pts, m.resolution)
    pose = np.array(truth, dtype=np.float64)

    def cycle(c):
        nonlocal pose
        pose = pose + np.array([0.0, 0.0, 0.001 if c % 2 else -0.001])
        f.force_update()
        return f.update(se2_from_xytheta(*pose), pts)

    for c in range(20):
        cycle(c)
    sample = f.particles()[0][:: max(1, f.num_particles() // 200)][:200]
    rates, kernel_ms = [], []
    for r in range(repeats):
        f.profile_enable(1)
        f.profile_read(reset=True)
        t0 = time.perf_counter()
        for c in range(cycles):
            cycle(c)
        dt = time.perf_counter() - t0
        prof = f.profile_read(reset=True)
        rates.append(cycles / dt)
        ms, cnt = prof["sensor_kernel"]
        kernel_ms.append(ms / cnt if cnt else float("nan"))
        f.profile_enable(0)
    out = {"case": name, "particles": f.num_particles(), "beams": beams, "K": int(len(means)), "map_cells": int(len(m.cells)),
           "present_per_lookup": round(present_per_lookup(m, sample, means), 3),
           "cycles_per_s_median": round(statistics.median(rates), 2), "cycles_per_s_min": round(min(rates), 2),
           "cycles_per_s_max": round(max(rates), 2), "ndt_kernel_ms_median": round(statistics.median(kernel_ms), 4),
           "ndt_kernel_ms_min": round(min(kernel_ms), 4), "ndt_kernel_ms_max": round(max(kernel_ms), 4)}
    f.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=50)
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "turtlebot3_world_grid.npz"))
    tb = load_ndt_map_npz(os.path.join(ROOT, "tests", "golden", "turtlebot3_world_ndt.npz"))
    run("config1_turtlebot", tb, z["cells"], float(z["resolution"]), tuple(z["origin_xytheta"][:2]), 500, 2000, 360, 3.5, a.repeats, a.cycles)
    cells = synth.make_rooms_map(4000, 4000, seed=42)
    keys, means, covs = synth.make_ndt_map(cells, 0.05, 1.0, origin_xy=(-100.0, -100.0), seed=1)
    run("synthetic_200m_1M", NDTMap2d(keys, means, covs, 1.0), cells, 0.05, (-100.0, -100.0), 1_000_000, 1_000_000, 1080, 30.0,
        a.repeats, a.cycles)


if __name__ == "__main__":
    main()
