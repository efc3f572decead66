"""The small landmark cycle (mcl_set_landmark_small_cycle) against a build of the PARENT commit, in alternating runs.

Lone filters of 2000 particles of each kind (landmark, bearing) with 6, 16 and 64 detections on two maps - the 43-landmark scene of
tests/test_gpu_landmark.py and a map of 1000 landmarks in 5 categories - and a fleet of 64 x 2000 landmark filters with 16 detections
behind mcl_landmark_batch_update.  Each measurement is a process of its own (a process loads one library): 20 warm-up cycles, then 5
repeats of 50 timed cycles.  The library under test runs with the switch on; the parent's build - named by --parent-lib and loaded
through BELUGA_MCL_LIB - has neither the switch nor the fleet call: its filters run the cycle they have, the fleet's one after the
other.  The rounds alternate parent, new, parent, new, ... so that a drift of the machine shows in both.  Writes
profiles/landmark_small_cycle.json.

    python tools/exp_landmark_small.py --parent-lib /path/to/parent/libbeluga_mcl.so [--rounds 3] [--repeats 5] [--cycles 50]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP = 20
FLEET, PARTICLES = 64, 2000
SENSOR_POSE = (0.0, 0.0, 0.0, 1.0, 0.1, 0.0, 0.5)
CASES = [f"{kind}-{world}-{k}" for kind in ("landmark", "bearing") for world in ("scene43", "wide1000") for k in (6, 16, 64)] + ["fleet-scene43-16"]


def world(name):
    """(positions, categories, box): scene43 is scene() of tests/test_gpu_landmark.py, wide1000 a map of 1000 landmarks in 5 categories."""
    import numpy as np
    if name == "scene43":
        rng = np.random.Generator(np.random.PCG64(1))
        pos = np.column_stack([rng.uniform(-10.0, 10.0, (40, 2)), rng.uniform(0.0, 2.0, 40)])
        cat = rng.integers(0, 5, 40).astype(np.uint32)
        pos = np.concatenate([pos, pos[:2], [[1.5, -2.5, 1.0]]])
        cat = np.concatenate([cat, cat[:2], [100]]).astype(np.uint32)
        return pos, cat, ((-12.0, -12.0, 0.0), (12.0, 12.0, 2.0))
    rng = np.random.Generator(np.random.PCG64(2))
    pos = np.column_stack([rng.uniform(-50.0, 50.0, (1000, 2)), rng.uniform(0.0, 2.0, 1000)])
    return pos, (np.arange(1000) % 5).astype(np.uint32), ((-52.0, -52.0, 0.0), (52.0, 52.0, 2.0))


def seen_from(pos, cat, pose, count, bearing, seed):
    """`count` landmarks (with repetition where the map has fewer) as seen from `pose`, with 2 cm of noise."""
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(seed))
    pick = rng.choice(len(pos), count, replace=count > len(pos))
    c, s = math.cos(pose[2]), math.sin(pose[2])
    v = pos[pick] - np.array([pose[0], pose[1], 0.0])
    local = np.column_stack([c * v[:, 0] + s * v[:, 1], c * v[:, 1] - s * v[:, 0], v[:, 2]])
    if bearing:
        local = local - np.asarray(SENSOR_POSE[4:])
        local = local / np.linalg.norm(local, axis=1)[:, None]
    return np.ascontiguousarray(local + rng.normal(0.0, 0.02, local.shape)), np.ascontiguousarray(cat[pick])


def child(case, switch, repeats, cycles):
    import numpy as np

    from beluga_amd.amcl import (Amcl, AmclBatch, AmclParams, BearingModelParam, DifferentialDriveModelParam, LandmarkMap, LandmarkMapBoundaries,
                                 LandmarkModelParam, se2_from_xytheta)

    kind, where, k = case.split("-")
    pos, cat, box = world(where)
    bearing = kind == "bearing"
    sensor = BearingModelParam(0.1, SENSOR_POSE) if bearing else LandmarkModelParam(sigma_range=0.4, sigma_bearing=0.15, random_prob=1e-3)
    motion = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
    lmap = LandmarkMap(LandmarkMapBoundaries(*box), (pos, cat))
    truth = (-0.5, 0.3, 0.2)
    det = seen_from(pos, cat, truth, int(k), bearing, 4)
    params = AmclParams(min_particles=PARTICLES, max_particles=PARTICLES)
    more = {"landmark_small_cycle": True} if switch else {}
    pose = np.array(truth, dtype=np.float64)
    if kind != "fleet":
        filters = [Amcl(lmap, motion, sensor, params, seed=3, **more)]
        batch = None
    elif switch:
        batch = AmclBatch([dict(grid=lmap, motion=motion, sensor=sensor, params=params, seed=100 + i, **more) for i in range(FLEET)])
        filters = batch.members
    else:  # (the parent has no fleet call for detections: 64 filters of their own, updated one after the other)
        filters = [Amcl(lmap, motion, sensor, params, seed=100 + i) for i in range(FLEET)]
        batch = None
    for f in filters:
        f.initialize(truth, np.diag([0.04, 0.04, 0.01]))

    def cycle(c):
        nonlocal pose
        pose = pose + np.array([0.0, 0.0, 0.001 if c % 2 else -0.001])
        ctrl = se2_from_xytheta(*pose)
        for f in filters:
            f.force_update()
        if batch is not None:
            batch.update_detections([ctrl] * FLEET, [det] * FLEET)
        else:
            for f in filters:
                f.update(ctrl, det)

    for c in range(WARMUP):
        cycle(c)
    rates = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for c in range(cycles):
            cycle(c)
        rates.append(cycles / (time.perf_counter() - t0))
    out = {"case": case, "switch": bool(switch), "cycles_per_s": [round(r, 2) for r in rates],
           "small_tail_launches": sum(f.counter("small_tail_launches") for f in filters)}
    if switch:
        out["landmark_wave_launches"] = sum(f.counter("landmark_wave_launches") for f in filters)
    if batch is not None:
        out.update({name: batch.counter(name) for name in ("kernel_launches", "landmark_launches", "members_landmark_fused", "members_alone")})
        batch.close()
    else:
        for f in filters:
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
    ap.add_argument("--cases", nargs="*", default=CASES, help="a subset of: " + " ".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "landmark_small_cycle.json"))
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

    result = {"warmup_cycles": WARMUP, "repeats": a.repeats, "cycles": a.cycles, "rounds": a.rounds, "particles": PARTICLES,
              "fleet_members": FLEET, "unit": "updates/s of the whole call as the Python caller sees it (a fleet: batch updates/s)", "cases": {}}
    for case in a.cases:
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
        with open(a.out, "w") as fh:  # (behind every case: a run that is cut short leaves what it measured)
            json.dump(result, fh, indent=1)
            fh.write("\n")
    print(json.dumps({c: {k: v for k, v in d.items() if k != "runs"} for c, d in result["cases"].items()}), flush=True)


if __name__ == "__main__":
    main()
