"""What mcl_estimate_clusters costs beside mcl_cluster_based_estimate: wall time per call, the calls alternating in one process on the
same set (the existing call is the yardstick; the difference is the price of the many-cluster pass and of the general path's launches).
One untimed round, then seven timed ones; medians and ranges.

    python tools/exp_cluster_modes.py [blobs_1m blobs_100k dispersed_1m small_2000]
"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from beluga_amd.amcl import Amcl, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam, OccupancyGrid, se2_from_xytheta

ROUNDS = 7
CENTRES = ((-40.0, -30.0, -2.0), (20.0, 10.0, 0.5), (60.0, -50.0, 2.5), (-10.0, 55.0, 1.0))


def four_blobs(n, seed=7):
    rng = np.random.Generator(np.random.PCG64(seed))
    c = np.asarray(CENTRES)[np.arange(n) * 4 // n]
    t = c[:, 2] + rng.normal(0.0, 0.1, n)
    states = np.stack([np.cos(t), np.sin(t), c[:, 0] + rng.normal(0.0, 0.15, n), c[:, 1] + rng.normal(0.0, 0.15, n)], axis=1)
    return states, rng.uniform(0.5, 1.5, n)


def measure(name, f):
    calls = {
        "cluster_based_estimate": lambda: f.cluster_based_estimate(),
        "estimate_clusters K=4": lambda: f.estimate_clusters(max_clusters=4),
        "estimate_clusters K=64": lambda: f.estimate_clusters(max_clusters=64),
        "count alone": lambda: f.estimate_clusters(max_clusters=0),
    }
    ms = {k: [] for k in calls}
    total = returned = 0
    for r in range(ROUNDS + 1):
        for k, call in calls.items():
            f.sync()
            t0 = time.perf_counter()
            got = call()
            dt = (time.perf_counter() - t0) * 1e3
            if r:
                ms[k].append(dt)
            if k == "estimate_clusters K=64":
                total, returned = got[0], len(got[1])
    print(f"{name}: {f.num_particles()} particles, {f.counter('cluster_cells')} cells, {total} clusters of more than one particle, {returned} returned",
          flush=True)
    for k, v in ms.items():
        print(f"  {k:26s} median {np.median(v):8.3f} ms   range {min(v):8.3f} .. {max(v):8.3f}", flush=True)


def main(which):
    cells, truth, _odoms, _scans, _poses = bench.make_workload(1)
    grid = OccupancyGrid(cells, bench.RESOLUTION, origin=se2_from_xytheta(bench.ORIGIN[0], bench.ORIGIN[1], 0.0))

    def new(n):
        return Amcl(grid, DifferentialDriveModelParam(*bench.ALPHAS), LikelihoodFieldModelParam(**bench.LF),
                    AmclParams(min_particles=n, max_particles=n), seed=42)
    for name, n in (("blobs_1m", 1_000_000), ("blobs_100k", 100_000), ("small_2000", 2000)):
        if name in which:
            f = new(n)
            f.set_particles(*four_blobs(n))
            measure(name, f)
            f.close()
    if "dispersed_1m" in which:
        f = new(1_000_000)
        f.initialize_from_map()
        measure("dispersed_1m", f)
        f.close()


if __name__ == "__main__":
    main(sys.argv[1:] or ["blobs_1m", "blobs_100k", "dispersed_1m", "small_2000"])
