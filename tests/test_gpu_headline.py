"""End-to-end parity AT the headline workloads: full `Amcl::update` cycles (amcl_core.hpp:165-201) of BASELINE configs[1]
(1M particles x 1080 beams, 4000x4000 @ 5 cm grid seed 42, resample every cycle - built by bench.py's own make_workload) and
of configs[2] (10M particles, KLD eps .05 z 3 + selective resampling) on the GPU against the oracle, cycle by cycle.

The stage tests of tests/test_gpu_parity.py check samples of full-size launches; these check the trajectory itself: the
estimate of every cycle, the weight normaliser, the policy decisions, the particle counts (exact) and the particle set at the
end.  Tolerances: estimates 1e-9 absolute (pose) / 1e-8 relative (covariance), normaliser 1e-11 relative; particle sets
identical except for CDF-boundary draws (the one index result that depends on the association of a prefix sum): each such
draw hands a slot another ancestor, whose descendants then differ - counted, bounded, and the estimate tolerance is widened by
what that many differing particles can move a mean over N.
"""
import math

import numpy as np
import pytest

import bench
from beluga_amd.amcl import (Amcl, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam, OccupancyGrid,
                             se2_from_xytheta)
from oracle import binding as orc

pytestmark = pytest.mark.gpu


def _filters(cells, params, seed=42):
    grid = OccupancyGrid(cells, bench.RESOLUTION, origin=se2_from_xytheta(bench.ORIGIN[0], bench.ORIGIN[1], 0.0))
    gpu = Amcl(grid, DifferentialDriveModelParam(*bench.ALPHAS), LikelihoodFieldModelParam(**bench.LF), params, seed=seed)
    lf = bench.LF
    cpu = orc.Amcl(min_particles=params.min_particles, max_particles=params.max_particles,
                   selective_resampling=params.selective_resampling, alphas=bench.ALPHAS, seed=seed, threads=orc.max_threads(),
                   lf=(lf["max_obstacle_distance"], lf["max_laser_distance"], lf["z_hit"], lf["z_random"], lf["sigma_hit"]),
                   lf_model_unknown_space=lf["model_unknown_space"])
    cpu.set_map(cells, bench.RESOLUTION, grid.origin)
    return grid, gpu, cpu


def _differing(gpu, cpu):
    """-> (particles whose state differs from the oracle's, the sum of their largest component differences: what they can move a
    sum over the set by)"""
    gs, gw = gpu.particles()
    cs, cw = cpu.particles()
    assert gs.shape == cs.shape
    assert np.array_equal(gw, cw) or np.allclose(gw, cw, rtol=1e-12, atol=0.0)
    delta = np.abs(gs - cs).max(axis=1)
    rows = delta > 1e-9
    return int(rows.sum()), float(delta[rows].sum())


def _check_cycle(c, g, o, gi, oi, n, differing_mass):
    assert (g is None) == (o is None), f"cycle {c}: update / no-update decisions differ"
    assert gi["resampled"] == oi["resampled"], f"cycle {c}: resample decisions differ"
    assert gi["weight_sum"] == pytest.approx(oi["weight_sum"], rel=1e-11), f"cycle {c}"
    # the differing particles move a mean over the n particles by at most the sum of their differences / n (second moments: times
    # the cloud's extent, metres at most - the factor 4)
    slack = differing_mass / n
    np.testing.assert_allclose(g[0], o[0], atol=1e-9 + slack, err_msg=f"cycle {c}: pose")
    np.testing.assert_allclose(g[1], o[1], rtol=1e-8, atol=1e-11 + 4.0 * slack, err_msg=f"cycle {c}: covariance")


def test_headline_config_1m_x_1080_over_the_timed_window_against_the_oracle():
    """BASELINE configs[1] exactly as bench.py builds and times it: 1M particles, 1080 beams, 4000^2 map (seed 42), multinomial
    resample every cycle, device-side recovery estimator, the LDS-patch kernel with its queue of blocks.  25 cycles = the driver's
    5 warm-up cycles and the 20 it times:
    the mix of patched, half-patched, gathered groups and of workgroups that gather everything changes over them as the cloud
    converges, and every cycle is compared - decisions, normaliser, estimate, the particle set."""
    cycles, n = 25, 1_000_000
    cells, truth, odoms, scans, _poses = bench.make_workload(cycles)
    params = AmclParams(min_particles=n, max_particles=n)
    grid, gpu, cpu = _filters(cells, params)
    cov = np.diag([0.25, 0.25, 0.04])
    gpu.initialize(truth, cov)
    cpu.initialize(truth, cov)
    planned0 = through0 = 0
    shares = []
    for c in range(cycles):
        ctrl = se2_from_xytheta(*odoms[c])
        g = gpu.update(ctrl, scans[c])
        o = cpu.update(ctrl, scans[c])
        gi, oi = gpu.last_info, cpu.last_info
        assert gi["num_particles"] == n == len(cpu.particles()[1])
        differing, mass = _differing(gpu, cpu)
        # CDF-boundary draws (<= 5 per cycle) and their descendants (a critical branching process: ~1 each on average)
        assert differing <= 10 * (c + 1), f"cycle {c}: {differing} particles differ from the oracle's set"
        _check_cycle(c, g, o, gi, oi, n, mass)
        assert gi["random_state_probability"] == pytest.approx(oi["random_state_probability"], abs=1e-12)
        # the kernel under test is the one the bench times: the LDS-patch kernel, its blocks from the queue, groups through patches
        # AND gathered ones in every cycle of the window
        assert gpu.counter("lf_patch_launches") == c + 1 and gpu.counter("lf_queue_launches") == c + 1
        planned, through = gpu.counter("lf_patch_groups_planned"), gpu.counter("lf_patch_groups_through")
        assert planned > planned0 and through > through0, f"cycle {c}: no group went through a patch"
        shares.append((through - through0) / (planned - planned0))
        planned0, through0 = planned, through
    assert min(shares) > 0.5 and shares[-1] > shares[0], shares  # (the cloud converges: more groups fit as the cycles go)
    assert any(s < 0.999 for s in shares[5:]), shares  # gathered groups are part of the timed window
    # and the filter localises: the estimate follows the true pose of the workload
    pose = _poses[cycles - 1]
    assert math.hypot(g[0][2] - pose[0], g[0][3] - pose[1]) < 0.25
    gpu.close()


def test_config3_10m_kld_selective_cycles_against_the_oracle():
    """BASELINE configs[2]: max 10M / min 100k particles, KLD (eps .05, z 3) + selective resampling (ESS < N/2), same map and
    scans.  The first cycle keeps all 10M particles (ESS above N/2: no resampling), the second takes the KLD cut; the particle
    count after every cycle is an integer result and must equal the oracle's."""
    cycles, n_max, n_min = 4, 10_000_000, 100_000
    cells, truth, odoms, scans, _poses = bench.make_workload(cycles)
    params = AmclParams(min_particles=n_min, max_particles=n_max, selective_resampling=True)
    grid, gpu, cpu = _filters(cells, params)
    cov = np.diag([0.25, 0.25, 0.04])
    gpu.initialize(truth, cov)
    cpu.initialize(truth, cov)
    counts, fired = [], []
    for c in range(cycles):
        ctrl = se2_from_xytheta(*odoms[c])
        g = gpu.update(ctrl, scans[c])
        o = cpu.update(ctrl, scans[c])
        gi, oi = gpu.last_info, cpu.last_info
        assert gi["num_particles"] == len(cpu.particles()[1]), f"cycle {c}: particle counts differ"
        counts.append(gi["num_particles"])
        fired.append(bool(gi["resampled"]))
        differing, mass = _differing(gpu, cpu)
        assert differing <= 5 * (c + 1), f"cycle {c}: {differing} particles differ from the oracle's set"
        _check_cycle(c, g, o, gi, oi, gi["num_particles"], mass)
        if oi["ess"] >= 0:
            assert gi["ess"] == pytest.approx(oi["ess"], rel=1e-10)
    assert counts[0] == n_max and not fired[0], (counts, fired)  # what bench.py reports as the cycle that does not fire
    assert any(fired) and n_min <= counts[-1] < n_max, (counts, fired)
    gpu.close()


def test_plain_bench_run_times_its_steps_and_dumps_the_last_estimate(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` without --full: ONE line with the headline's fields and nothing
    measured beside them, `ms_per_step` = the timed region over exactly K steps, and in DIR the estimate that the last timed update
    returned - the one a filter in this process returns after W + K cycles on the same seeded inputs."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    steps, warmup, n = 3, 2, 1_000_000
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--dump-outputs", str(out_dir)]
    run = subprocess.run(cmd, capture_output=True, text=True, cwd=root, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, run.stdout
    line = json.loads(lines[0])
    assert line["metric"] == "MCL update cycles/sec (motion+sensor+resample), N particles x 1080 beams"
    assert line["unit"] == "cycles/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == steps and line["warmup"] == warmup and line["config"]["particles_total"] == n
    assert line["ms_per_step"] == pytest.approx(line["timed_region_s"] / steps * 1e3, rel=1e-9)
    assert line["value"] == pytest.approx(steps / line["timed_region_s"], rel=1e-9)
    for key in ("repeat_windows", "stage_ms", "roofline", "roofline_by_kernel", "verified", "configs", "cpu_baseline"):
        assert key not in line, f"{key}: only with --full"
    pose, cov = np.load(out_dir / "pose.npy"), np.load(out_dir / "covariance.npy")
    assert pose.dtype == np.float64 and pose.shape == (4,) and cov.dtype == np.float64 and cov.shape == (3, 3)

    cells, truth, odoms, scans, _poses = bench.make_workload(warmup + steps)
    grid = OccupancyGrid(cells, bench.RESOLUTION, origin=se2_from_xytheta(bench.ORIGIN[0], bench.ORIGIN[1], 0.0))
    gpu = Amcl(grid, DifferentialDriveModelParam(*bench.ALPHAS), LikelihoodFieldModelParam(**bench.LF),
               AmclParams(min_particles=n, max_particles=n), seed=42)
    gpu.initialize(truth, np.diag([0.25, 0.25, 0.04]))
    for c in range(warmup + steps):
        g = gpu.update(se2_from_xytheta(*odoms[c]), scans[c])
        assert g is not None
    gpu.close()
    np.testing.assert_allclose(pose, g[0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(cov, g[1], rtol=1e-10, atol=1e-15)
