"""The beam model over a range table, measured: speed against a build of the PARENT commit on the exact beam path, and what the
approximation costs.

Speed.  One child process per (build, shape), this build with a table and the parent build (--parent-lib: its libbeluga_mcl.so, loaded
through BELUGA_MCL_LIB) on the exact path, in ALTERNATING runs on one box, as tools/exp_ndt_small.py does.  A child initialises the
filter around a free pose, runs `warmup` cycles and times `steps` cycles (host wall time, stream idle at the end) and the sensor kernel
(profiling level 1).  Shapes: 1M x 1080 and 2000 x 180 on the turtlebot map (3.5 m reach), 1M x 1080 on the synthetic 4096 x 4096 map
(30 m reach; A = 120 and A = 360).  The table's build time and bytes are recorded per shape.

Cost.  On the turtlebot map, A in {90, 180, 360, 720}: 10^5 poses uniform over free space, a scan synthesised by mcl_cast_rays from a true
pose; median, 99th percentile and maximum of |log L_table - log L_exact| from mcl_likelihoods on a table context and on an exact twin;
and the final pose error of a 40-cycle run of each.  Recorded, not gated.

    python tools/exp_range_table.py --parent-lib PATH [--rounds 3] [--out profiles/range_table.json]
    (each child is started under `timeout`; a child that fails ends the run)
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {  # name: (map, particles, beams, max_range, A, warmup, steps)
    "turtlebot_1M_x_1080_A360": ("turtlebot", 1_000_000, 1080, 3.5, 360, 3, 10),
    "turtlebot_2000_x_180_A360": ("turtlebot", 2000, 180, 3.5, 360, 20, 200),
    "synthetic4096_1M_x_1080_A120": ("synthetic", 1_000_000, 1080, 30.0, 120, 3, 10),
    "synthetic4096_1M_x_1080_A360": ("synthetic", 1_000_000, 1080, 30.0, 360, 3, 10),
}


def load_map(name):
    from beluga_amd import synth
    from beluga_amd.amcl import OccupancyGrid, se2_from_xytheta

    if name == "turtlebot":
        z = np.load(os.path.join(ROOT, "tests", "golden", "turtlebot3_world_grid.npz"))
        ox, oy, ot = z["origin_xytheta"]
        return OccupancyGrid(cells=z["cells"], resolution=float(z["resolution"]), origin=se2_from_xytheta(ox, oy, ot))
    return OccupancyGrid(cells=synth.make_rooms_map(4096, 4096, seed=42), resolution=0.05, origin=se2_from_xytheta(-102.4, -102.4, 0.0))


def make_filter(grid, n, max_range, seed=3):
    from beluga_amd.amcl import Amcl, AmclParams, BeamModelParam, DifferentialDriveModelParam

    params = AmclParams(min_particles=n, max_particles=n, update_min_d=0.0, update_min_a=0.0, resample_interval=1)
    # (the 4 GiB default holds 4096 x 4096 x 64 bins: the synthetic shapes ask for more)
    return Amcl(grid, DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05), BeamModelParam(0.5, 0.05, 0.05, 0.5, 0.2, 0.1, max_range), params, seed=seed)


def child_speed(shape, table):
    from beluga_amd import synth
    from beluga_amd.amcl import se2_from_xytheta

    map_name, n, B, max_range, A, warmup, steps = SHAPES[shape]
    grid = load_map(map_name)
    truth = synth.find_free_pose(grid.cells, grid.resolution, (grid.origin[2], grid.origin[3]), seed=2, clearance_cells=4)
    f = make_filter(grid, n, max_range)
    f.initialize(truth, np.diag([0.05, 0.05, 0.02]))
    out = {"shape": shape, "table": bool(table)}
    if table:
        f.set_option("range_table_max_bytes", 1 << 36)
        t0 = time.perf_counter()
        f.build_range_table(A)
        out["build_ms"] = (time.perf_counter() - t0) * 1e3
        out["table_bytes"] = f.range_table_info()["bytes"]
    angles = -math.pi + 2 * math.pi * np.arange(B) / B
    pose_c = np.array([[math.cos(truth[2]), math.sin(truth[2]), truth[0], truth[1]]])
    ranges = f.cast_rays(pose_c, angles=angles, max_range=max_range)[0]
    pts = np.stack([ranges * np.cos(angles), ranges * np.sin(angles)], axis=1)
    pts = pts[ranges < max_range] if (ranges < max_range).sum() >= B // 2 else pts
    out["beams_used"] = len(pts)
    odom = [0.0, 0.0, 0.0]

    def cycle():
        odom[0] += 0.001
        f.update(se2_from_xytheta(*odom), pts)

    for _ in range(warmup):
        cycle()
    f.sync()
    f.profile_enable(1)
    t0 = time.perf_counter()
    for _ in range(steps):
        cycle()
    f.sync()
    out["cycle_ms"] = (time.perf_counter() - t0) / steps * 1e3
    out["cycles_per_s"] = 1e3 / out["cycle_ms"]
    ms, count = f.profile_read()["sensor_kernel"]  # (level 1 samples the sensor kernel of some cycles only)
    out["sensor_kernel_ms"] = ms / count if count else None
    if table:
        out["lut_launches"] = f.range_table_info()["lut_launches"]
    f.close()
    print("RESULT " + json.dumps(out), flush=True)


def child_cost():
    from beluga_amd import synth
    from beluga_amd.amcl import se2_from_xytheta

    grid = load_map("turtlebot")
    max_range, B, n = 3.5, 360, 100_000
    truth = synth.find_free_pose(grid.cells, grid.resolution, (grid.origin[2], grid.origin[3]), seed=2, clearance_cells=4)
    rng = np.random.Generator(np.random.PCG64(11))
    free = np.argwhere(np.asarray(grid.cells) == 0)
    pick = free[rng.integers(0, len(free), n)]
    gx, gy = (pick[:, 1] + rng.uniform(0, 1, n)) * grid.resolution, (pick[:, 0] + rng.uniform(0, 1, n)) * grid.resolution
    oc, os_, ox, oy = grid.origin
    th = rng.uniform(-math.pi, math.pi, n)
    poses = np.ascontiguousarray(np.stack([np.cos(th), np.sin(th), oc * gx - os_ * gy + ox, os_ * gx + oc * gy + oy], axis=1))
    exact = make_filter(grid, 2000, max_range, seed=5)
    angles = -math.pi + 2 * math.pi * np.arange(B) / B

    def scan_at(pose):
        pose_c = np.array([[math.cos(pose[2]), math.sin(pose[2]), pose[0], pose[1]]])
        r = exact.cast_rays(pose_c, angles=angles, max_range=max_range)[0]
        keep = r < max_range
        return np.stack([r[keep] * np.cos(angles[keep]), r[keep] * np.sin(angles[keep])], axis=1)

    pts = scan_at(truth)
    log_exact = np.log(exact.likelihoods(poses, pts))
    out = {"poses": n, "beams": len(pts), "rows": []}

    def run(f):
        f.initialize(truth, np.diag([0.05, 0.05, 0.02]))
        pose, odom, est = truth, (0.0, 0.0, 0.0), None
        for c in range(40):
            pose, odom = synth.odometry_step(pose, 0.05, 0.02), synth.odometry_step(odom, 0.05, 0.02)
            r = f.update(se2_from_xytheta(*odom), scan_at(pose))
            est = r[0] if r is not None else est
        return float(math.hypot(est[2] - pose[0], est[3] - pose[1])), float(abs(math.atan2(math.sin(math.atan2(est[1], est[0]) - pose[2]),
                                                                                             math.cos(math.atan2(est[1], est[0]) - pose[2]))))

    out["exact_final_error_m_rad"] = run(make_filter(grid, 2000, max_range, seed=9))
    for A in (90, 180, 360, 720):
        f = make_filter(grid, 2000, max_range, seed=9)
        f.build_range_table(A)
        d = np.abs(np.log(f.likelihoods(poses, pts)) - log_exact)
        row = {"A": A, "median": float(np.median(d)), "p99": float(np.percentile(d, 99)), "max": float(d.max()), "final_error_m_rad": run(f)}
        out["rows"].append(row)
        f.close()
    exact.close()
    print("RESULT " + json.dumps(out), flush=True)


def spawn(args, env_extra, limit):
    env = dict(os.environ, **env_extra)
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        raise SystemExit("child %s ended with %d: nothing more is started" % (args, p.returncode))
    return json.loads([l for l in p.stdout.split("\n") if l.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--no-cost", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_table.json"))
    ap.add_argument("--child")
    ap.add_argument("--table", type=int, default=0)
    args = ap.parse_args()
    if args.child == "cost":
        return child_cost()
    if args.child:
        return child_speed(args.child, args.table)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's libbeluga_mcl.so is needed (the exact path is measured on ITS build)")
    record = {"what": "beam model over a range table (this build) against the exact beam path of the parent commit's build; alternating child "
                      "processes on one box; cycle_ms: host wall time per mcl_update, stream idle at the end; sensor_kernel_ms: profiling level 1",
              "rounds": args.rounds, "speed": [], "cost": None}
    for shape in args.shapes.split(","):
        runs = {"table": [], "parent_exact": []}
        for _ in range(args.rounds):
            runs["table"].append(spawn(["--child", shape, "--table", "1"], {}, 400))
            runs["parent_exact"].append(spawn(["--child", shape, "--table", "0"], {"BELUGA_MCL_LIB": os.path.abspath(args.parent_lib)}, 400))
        row = {"shape": shape, "runs": runs}
        for k, v in runs.items():
            row[k + "_cycle_ms"] = statistics.median(r["cycle_ms"] for r in v)
            kernel = [r["sensor_kernel_ms"] for r in v if r["sensor_kernel_ms"] is not None]
            row[k + "_sensor_kernel_ms"] = statistics.median(kernel) if kernel else None
        row["cycle_speedup"] = row["parent_exact_cycle_ms"] / row["table_cycle_ms"]
        if row["parent_exact_sensor_kernel_ms"] and row["table_sensor_kernel_ms"]:
            row["sensor_kernel_speedup"] = row["parent_exact_sensor_kernel_ms"] / row["table_sensor_kernel_ms"]
        row["build_ms"] = statistics.median(r["build_ms"] for r in runs["table"])
        row["table_bytes"] = runs["table"][0]["table_bytes"]
        record["speed"].append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "runs"}), flush=True)
        with open(args.out, "w") as fh:  # (what is measured so far survives a later child's failure)
            json.dump(record, fh, indent=1)
            fh.write("\n")
    if not args.no_cost:
        record["cost"] = spawn(["--child", "cost"], {}, 400)
        print(json.dumps(record["cost"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
