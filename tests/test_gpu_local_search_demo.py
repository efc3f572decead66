"""tests/cpp/local_search_demo.cpp: Amcl::local_search and relocalize with refinement of the C++ facade, and ros::Amcl::local_search over a
laser scan - their hits equal the Python facade's on the same map, scan and seeds, bit for bit (all are the same call of the C ABI),
and the estimate after the refined relocalize stays at the best hit's mean pose."""
import math
import os
import subprocess

import numpy as np
import pytest

from beluga_amd import build as mcl_build
from beluga_amd.amcl import Amcl, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam, OccupancyGrid, se2_from_xytheta

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fields(h):
    return [h.di, h.dj, h.dk, h.plateau, h.score, h.seed_score, h.pose[2], h.pose[3], h.pose[0], h.pose[1], h.mean_pose[2], h.mean_pose[3],
            h.cov[0, 0], h.cov[1, 1], h.cov[2, 2]]


def test_cpp_demo_hits_equal_the_python_facades(tmp_path):
    mcl_build.build()
    exe, lib_dir = str(tmp_path / "local_search_demo"), os.path.join(ROOT, "beluga_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "local_search_demo.cpp"), "-L", lib_dir, "-lbeluga_mcl", f"-Wl,-rpath,{lib_dir}", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    parsed = {tag: [[int(v) for v in l.split()[1:5]] + [float(v) for v in l.split()[5:]] for l in lines if l.startswith(tag + " ")]
              for tag in ("hit", "refined", "ros_hit")}
    estimate = [np.array(l.split()[1:], dtype=np.float64) for l in lines if l.startswith("estimate ")]
    assert 1 <= len(parsed["hit"]) <= 5 and len(estimate) == 1
    W, H = 64, 48
    cells = np.zeros((H, W), dtype=np.int8)
    cells[0, :] = cells[-1, :] = cells[:, 0] = cells[:, -1] = 100
    cells[30, [x for x in range(W) if x < 12 or x > 18]] = 100
    cells[:30, 40] = 100
    grid = OccupancyGrid(cells=cells, resolution=0.1, origin=se2_from_xytheta(-1.0, -1.0, 0.0))
    lf = LikelihoodFieldModelParam(max_obstacle_distance=2.0, max_laser_distance=100.0)
    scan = np.array([[3.0, 0.0], [0.0, 2.0], [-1.0, 0.0], [0.0, -1.0], [3.0, 1.0], [3.0, -1.0], [1.0, 2.0], [-1.0, 1.0]])
    f = Amcl(grid, DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05), lf, AmclParams(min_particles=300, max_particles=1500), seed=5)
    coarse = f.global_search(scan, headings=36, max_results=5)
    want = f.local_search(np.array([h.pose for h in coarse]), scan)
    refined = f.relocalize(scan, refine={}, headings=36, max_results=5)
    f.close()
    for tag, expected in (("hit", want), ("ros_hit", want), ("refined", refined)):
        assert parsed[tag] == [fields(h) for h in expected], tag  # (%.17g round-trips a double: equal floats are equal bits)
    best = refined[0]
    assert math.hypot(estimate[0][0] - best.mean_pose[2], estimate[0][1] - best.mean_pose[3]) < 0.3
