"""The small NDT cycle (mcl_set_ndt_small_cycle) against a build of the PARENT commit, in alternating runs.

Two cases: the turtlebot NDT case of tools/exp_ndt.py (config 1: KLD 500 .. 2000 particles, 360 beams) as a lone filter, and a fleet of
64 NDT filters of 2000 particles behind mcl_batch_update.  Each measurement is a process of its own (a process loads one library): 20
warm-up cycles, then 5 repeats of 50 timed cycles.  The library under test runs with the switch on; the parent's build - named by
--parent-lib and loaded through BELUGA_MCL_LIB - has no switch and runs the cycle it has.  The rounds alternate parent, new, parent,
new, ... so that a drift of the machine shows in both.  Writes profiles/ndt_small_cycle.json.

    python tools/exp_ndt_small.py --parent-lib /path/to/parent/libbeluga_mcl.so [--rounds 3] [--repeats 5] [--cycles 50]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP = 20
FLEET, FLEET_PARTICLES = 64, 2000


def child(case, switch, repeats, cycles):
    import numpy as np

    from beluga_amd import synth
    from beluga_amd.amcl import (Amcl, AmclBatch, AmclParams, DifferentialDriveModelParam, NDTModelParam2d, load_ndt_map_npz,
                                 se2_from_xytheta)

    node = NDTModelParam2d(minimum_likelihood=0.01, d1=1.0, d2=0.6)
    motion = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
    z = np.load(os.path.join(ROOT, "tests", "golden", "turtlebot3_world_grid.npz"))
    tb = load_ndt_map_npz(os.path.join(ROOT, "tests", "golden", "turtlebot3_world_ndt.npz"))
    cells, res, origin = z["cells"], float(z["resolution"]), tuple(z["origin_xytheta"][:2])
    truth = synth.find_free_pose(cells, res, origin, seed=4, clearance_cells=10)
    angles = synth.lidar_angles(360, 360.0)
    pts = synth.scan_points(synth.cast_scan(cells, res, origin, truth, angles, 3.5, 0.01, seed=1), angles)
    more = {"ndt_small_cycle": True} if switch else {}
    pose = np.array(truth, dtype=np.float64)
    if case == "turtlebot":
        f = Amcl(tb, motion, node, AmclParams(min_particles=500, max_particles=2000), seed=3, **more)
        f.initialize(truth, np.diag([0.04, 0.04, 0.01]))

        def cycle(c):
            nonlocal pose
            pose = pose + np.array([0.0, 0.0, 0.001 if c % 2 else -0.001])
            f.force_update()
            f.update(se2_from_xytheta(*pose), pts)

        def counts():
            return {"small_cycles_in_tail": f.ndt_small_cycle_counts()[0], "small_cycles_handed_back": f.ndt_small_cycle_counts()[1],
                    "particles": f.num_particles()} if switch else {"particles": f.num_particles()}
    else:
        params = AmclParams(min_particles=FLEET_PARTICLES, max_particles=FLEET_PARTICLES)
        f = AmclBatch([dict(grid=tb, motion=motion, sensor=node, params=params, seed=100 + i, **more) for i in range(FLEET)])
        for m in f.members:
            m.initialize(truth, np.diag([0.04, 0.04, 0.01]))
        scans = [pts] * FLEET

        def cycle(c):
            nonlocal pose
            pose = pose + np.array([0.0, 0.0, 0.001 if c % 2 else -0.001])
            for m in f.members:
                m.force_update()
            f.update([se2_from_xytheta(*pose)] * FLEET, scans)

        def counts():
            out = {"members_fused": f.counter("members_fused"), "members_alone": f.counter("members_alone"),
                   "kernel_launches": f.counter("kernel_launches")}
            if switch:
                out["ndt_launches"], out["members_ndt_fused"] = f.ndt_counts()
                out["small_cycles_handed_back"] = sum(m.ndt_small_cycle_counts()[1] for m in f.members)
            return out

    for c in range(WARMUP):
        cycle(c)
    rates = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for c in range(cycles):
            cycle(c)
        rates.append(cycles / (time.perf_counter() - t0))
    out = {"case": case, "switch": bool(switch), "cycles_per_s": [round(r, 2) for r in rates]}
    out.update(counts())
    f.close()
    print(json.dumps(out), flush=True)


def spread(values):
    return {"median": round(statistics.median(values), 2), "min": round(min(values), 2), "max": round(max(values), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libbeluga_mcl.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ndt_small_cycle.json"))
    ap.add_argument("--child", nargs=2, metavar=("CASE", "SWITCH"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1] == "1", a.repeats, a.cycles)
        return
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        ap.error("--parent-lib: a build of the parent commit is what the switch is measured against")

    def measure(case, new):
        env = dict(os.environ)
        env.pop("BELUGA_MCL_LIB", None)
        if not new:
            env["BELUGA_MCL_LIB"] = os.path.abspath(a.parent_lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "1" if new else "0", "--repeats", str(a.repeats),
               "--cycles", str(a.cycles)]
        done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
        if done.returncode != 0:  # nothing more is started on the device behind a failed run
            sys.exit(f"{case} ({'new' if new else 'parent'}) ended with status {done.returncode}:\n{done.stderr[-2000:]}")
        return json.loads(done.stdout.strip().splitlines()[-1])

    result = {"warmup_cycles": WARMUP, "repeats": a.repeats, "cycles": a.cycles, "rounds": a.rounds, "cases": {}}
    for case in ("turtlebot", "fleet"):
        runs = {"parent": [], "new": []}
        for r in range(a.rounds):
            for which in ("parent", "new"):
                run = measure(case, which == "new")
                runs[which].append(run)
                print(json.dumps({"round": r, "build": which, **run}), flush=True)
        medians = {w: [statistics.median(run["cycles_per_s"]) for run in runs[w]] for w in runs}
        ratios = [n / p for n, p in zip(medians["new"], medians["parent"])]  # round by round: neighbours in time
        result["cases"][case] = {
            "parent_cycles_per_s": spread([v for run in runs["parent"] for v in run["cycles_per_s"]]),
            "new_cycles_per_s": spread([v for run in runs["new"] for v in run["cycles_per_s"]]),
            "ratio_new_over_parent": {"median": round(statistics.median(ratios), 3), "min": round(min(ratios), 3), "max": round(max(ratios), 3)},
            "every_new_run_above_every_parent_run": min(medians["new"]) > max(medians["parent"]),
            "runs": runs,
        }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps({c: {k: v for k, v in d.items() if k != "runs"} for c, d in result["cases"].items()}), flush=True)


if __name__ == "__main__":
    main()
