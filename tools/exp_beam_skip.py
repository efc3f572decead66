"""What beam skipping costs (DESIGN.md "Beam skipping"): bench.py's workload - 1M particles x 1080 beams on the 4000 x 4000 rooms map -
and a small filter, 2000 particles x 180 beams of the same scans, as update cycles per second of

    parent   a build of the commit before the feature (--parent-lib; loaded through BELUGA_MCL_LIB), skipping unknown to it
    off      this build, skipping off
    on       this build, skipping on with Nav2's defaults

Every figure comes from a fresh child process; the three take turns, round after round (parent, off, on, parent, ...), so that drift
of the machine falls on all alike.  Reported per size: every round's figure, the median, the spread (max - min) / median of each,
and - from a short run with stage profiling on, HIP events on the filter's stream - the time of MCL_STAGE_REWEIGHT with skipping on
and off (the stage holds the count, its synchronisation and the reweight) beside the wall time of one mcl_beam_agreement call.
Writes profiles/beam_skip.json.

    python tools/exp_beam_skip.py --parent-lib /path/to/parent/libbeluga_mcl.so [--rounds 3] [--steps 120] [--out profiles/beam_skip.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP = 20
SIZES = {"1M_x_1080": (1_000_000, 1), "2000_x_180": (2000, 6)}  # particles, every k-th beam of the 1080


def child(mode, steps):
    import bench
    from beluga_amd.amcl import Amcl, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam, OccupancyGrid, se2_from_xytheta
    cells, truth, odoms, scans, _ = bench.make_workload(WARMUP + steps)
    grid = OccupancyGrid(cells, bench.RESOLUTION, origin=se2_from_xytheta(bench.ORIGIN[0], bench.ORIGIN[1], 0.0))
    controls = [se2_from_xytheta(*o) for o in odoms]
    out = {}
    for name, (n, every) in SIZES.items():
        pts = [np.ascontiguousarray(s[::every]) for s in scans]
        f = Amcl(grid, DifferentialDriveModelParam(*bench.ALPHAS), LikelihoodFieldModelParam(**bench.LF), AmclParams(min_particles=n, max_particles=n), seed=42)
        if mode == "on":
            f.set_beam_skip(True)
        f.initialize(truth, np.diag([0.25, 0.25, 0.04]))
        for c in range(WARMUP):
            f.update(controls[c], pts[c])
        f.sync()
        t0 = time.perf_counter()
        for c in range(WARMUP, WARMUP + steps):
            f.update(controls[c], pts[c])
        f.sync()
        r = {"cycles_per_s": steps / (time.perf_counter() - t0)}
        if mode != "parent":
            r["used_all"], r["count_launches"] = f.counter("beam_skip_used_all"), f.counter("beam_skip_launches")
            t0 = time.perf_counter()
            for _ in range(10):
                f.beam_agreement(pts[0])
            r["beam_agreement_call_ms"] = (time.perf_counter() - t0) / 10 * 1e3
            f.profile_enable(2)
            for c in range(WARMUP, WARMUP + 10):
                f.force_update()
                f.update(controls[c], pts[c])
            ms, count = f.profile_read()["reweight"]
            r["stage_reweight_ms"] = ms / max(count, 1)
        f.close()
        out[name] = r
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_skip.json"))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.steps)
    modes = (["parent"] if args.parent_lib else []) + ["off", "on"]
    runs = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            env = dict(os.environ)
            if m == "parent":
                env["BELUGA_MCL_LIB"] = args.parent_lib
            text = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", m, "--steps", str(args.steps)], env=env, check=True,
                                  capture_output=True, text=True, timeout=600).stdout
            runs[m].append(json.loads([line for line in text.splitlines() if line.startswith("RESULT ")][-1][7:]))
            print(m, json.dumps(runs[m][-1]), flush=True)
    results = {}
    for size in SIZES:
        results[size] = {}
        for m in modes:
            v = [r[size]["cycles_per_s"] for r in runs[m]]
            entry = {"cycles_per_s_rounds": v, "cycles_per_s": statistics.median(v), "spread": (max(v) - min(v)) / statistics.median(v)}
            for key in ("stage_reweight_ms", "beam_agreement_call_ms", "used_all", "count_launches"):
                if key in runs[m][0][size]:
                    entry[key] = statistics.median(r[size][key] for r in runs[m])
            results[size][m] = entry
    record = {"what": "update cycles per second with beam skipping unknown (parent build), off and on; fresh processes in alternating rounds; "
                      "stage_reweight_ms: HIP events around MCL_STAGE_REWEIGHT (count + synchronisation + reweight when on), profiling level 2",
              "rounds": args.rounds, "steps": args.steps, "warmup": WARMUP, "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(json.dumps(results, indent=1))


if __name__ == "__main__":
    main()
