"""Times the NDT map build on the device against the host route on the same input, in the same process.

    python tools/exp_ndt_build.py [--repeats 7]

Two inputs: a seeded cloud of 10^6 points over the 200 m x 200 m extent of the benchmark map at 1 m cells, and the occupied cells of
the 4000 x 4000 benchmark grid (synth.make_rooms_map, seed 42, 5 cm) at 1 m cells.  Per input and route: one untimed run, then
`repeats` timed ones, alternating the routes; wall time of the whole call (upload, kernels and the synchronisation at the end of the
device route; the fit, the layout and the upload of the host route).  Prints the median and the range of each, one JSON line at the end.

  device route : mcl_build_ndt_map_from_points / mcl_build_ndt_map_from_grid
  host route   : mcl_ndt_measurement_cells + the keys (NDTMap2d.from_points), then mcl_set_ndt_map; for the grid the cell centres
                 are computed with numpy first (occupied_cell_centres), which is part of what a caller without the device route does
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from beluga_amd import synth  # noqa: E402
from beluga_amd.amcl import (Amcl, AmclParams, DifferentialDriveModelParam, NDTMap2d, NDTModelParam2d, OccupancyGrid,  # noqa: E402
                             occupied_cell_centres, se2_from_xytheta)


def timed(fn, sync):
    sync()
    t = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    start = NDTMap2d(np.array([[0, 0]], dtype=np.int32), np.array([[0.5, 0.5]]), np.eye(2)[None] * 0.1, 1.0)
    f = Amcl(start, DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05), NDTModelParam2d(0.01, 1.0, 0.6), AmclParams(min_particles=100, max_particles=100))
    cloud = np.random.Generator(np.random.PCG64(2026)).uniform(-100.0, 100.0, (1_000_000, 2))
    grid = OccupancyGrid(cells=synth.make_rooms_map(4000, 4000, seed=42), resolution=0.05, origin=se2_from_xytheta(-100.0, -100.0, 0.0))
    inputs = {
        "cloud_1M": (lambda: f.build_ndt_map(cloud, 1.0), lambda: f.update_map(NDTMap2d.from_points(cloud, 1.0)), len(cloud)),
        "grid_4000": (lambda: f.build_ndt_map(grid, 1.0), lambda: f.update_map(NDTMap2d.from_points(occupied_cell_centres(grid), 1.0)),
                      int(np.count_nonzero(grid.cells == 100))),
    }
    out = {}
    for name, (device, host, points) in inputs.items():
        device()
        built = f.ndt_map()
        host()
        given = f.ndt_map()
        same = bool(np.array_equal(built.cells, given.cells) and np.array_equal(built.means, given.means) and
                    np.array_equal(built.covariances, given.covariances))
        d, h = [], []
        for _ in range(a.repeats):
            d.append(timed(device, f.sync))
            h.append(timed(host, f.sync))
        out[name] = {"points": points, "cells": len(built.cells), "same_cells": same,
                     "device_ms": {"median": float(np.median(d)), "min": min(d), "max": max(d)},
                     "host_ms": {"median": float(np.median(h)), "min": min(h), "max": max(h)}}
        print(f"{name}: {points} points -> {len(built.cells)} cells (equal: {same}); device {np.median(d):.2f} ms [{min(d):.2f} .. {max(d):.2f}], "
              f"host {np.median(h):.2f} ms [{min(h):.2f} .. {max(h):.2f}]", flush=True)
    f.close()
    print(json.dumps({"exp_ndt_build": out, "repeats": a.repeats}))


if __name__ == "__main__":
    main()
