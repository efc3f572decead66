"""Landmark and bearing sensor models: cycles/s of the whole update and the sensor kernel's time (HIP events around it, profile level
1), at 1M particles x 16 detections over 256 landmarks in 8 categories (32 candidates per detection), for both models, and at 2000
particles KLD-adaptive (500 .. 2000) on the same scene.  20 warm-up cycles, then `repeats` x `cycles` timed; median and range.

    python tools/exp_landmark.py [--repeats 5] [--cycles 50]
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

from beluga_amd.amcl import (Amcl, AmclParams, BearingModelParam, DifferentialDriveModelParam, LandmarkMap, LandmarkMapBoundaries,  # noqa: E402
                             LandmarkModelParam, se2_from_xytheta)

SENSOR_HEIGHT = 0.5


def scene(seed=1, landmarks=256, categories=8, extent=40.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    pos = np.column_stack([rng.uniform(-extent / 2, extent / 2, (landmarks, 2)), rng.uniform(0.2, 2.0, landmarks)])
    cat = (np.arange(landmarks) % categories).astype(np.uint32)
    half = extent / 2 + 2.0
    return pos, cat, LandmarkMapBoundaries((-half, -half, 0.0), (half, half, 2.0))


def seen_from(pos, cat, pose, count, bearing):
    """The `count` landmarks nearest to `pose`, as positions in the robot frame or as unit bearings from the sensor above it."""
    order = np.argsort(np.hypot(pos[:, 0] - pose[0], pos[:, 1] - pose[1]))[:count]
    c, s = math.cos(pose[2]), math.sin(pose[2])
    v = pos[order] - np.array([pose[0], pose[1], 0.0])
    local = np.column_stack([c * v[:, 0] + s * v[:, 1], c * v[:, 1] - s * v[:, 0], v[:, 2]])
    if bearing:
        local = local - np.array([0.0, 0.0, SENSOR_HEIGHT])
        local = local / np.linalg.norm(local, axis=1)[:, None]
    return local, cat[order]


def run(name, bearing, n_min, n_max, detections, repeats, cycles):
    pos, cat, box = scene()
    sensor = (BearingModelParam(0.1, (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, SENSOR_HEIGHT)) if bearing
              else LandmarkModelParam(sigma_range=0.3, sigma_bearing=0.15, random_prob=1e-3))
    f = Amcl(LandmarkMap(box, (pos, cat)), DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05), sensor,
             AmclParams(min_particles=n_min, max_particles=n_max), seed=3)
    truth = (1.0, -2.0, 0.3)
    f.initialize(truth, np.diag([0.04, 0.04, 0.01]))
    det = seen_from(pos, cat, truth, detections, bearing)
    pose = np.array(truth, dtype=np.float64)

    def cycle(c):
        nonlocal pose
        pose = pose + np.array([0.0, 0.0, 0.001 if c % 2 else -0.001])
        f.force_update()
        return f.update(se2_from_xytheta(*pose), det)

    for c in range(20):
        cycle(c)
    rates, kernel_ms = [], []
    for _ in range(repeats):
        f.profile_enable(1)
        f.profile_read(reset=True)
        t0 = time.perf_counter()
        for c in range(cycles):
            cycle(c)
        dt = time.perf_counter() - t0
        ms, cnt = f.profile_read(reset=True)["sensor_kernel"]
        rates.append(cycles / dt)
        kernel_ms.append(ms / cnt if cnt else float("nan"))
        f.profile_enable(0)
    out = {"case": name, "model": "bearing" if bearing else "landmark", "particles": f.num_particles(), "detections": detections,
           "landmarks": len(pos), "categories": int(cat.max()) + 1,
           "cycles_per_s_median": round(statistics.median(rates), 2), "cycles_per_s_min": round(min(rates), 2),
           "cycles_per_s_max": round(max(rates), 2), "kernel_ms_median": round(statistics.median(kernel_ms), 4),
           "kernel_ms_min": round(min(kernel_ms), 4), "kernel_ms_max": round(max(kernel_ms), 4)}
    f.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=50)
    a = ap.parse_args()
    for bearing in (False, True):
        run("kld_500_2000", bearing, 500, 2000, 16, a.repeats, a.cycles)
        run("fixed_1M", bearing, 1_000_000, 1_000_000, 16, a.repeats, a.cycles)


if __name__ == "__main__":
    main()
