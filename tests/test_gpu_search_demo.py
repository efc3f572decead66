"""tests/cpp/search_demo.cpp: Amcl::global_search and relocalize of the C++ facade, and ros::Amcl::global_search over a laser scan - their
hits equal the Python facade's on the same map and scan, bit for bit (all are the same call of the C ABI), and the estimate after
relocalize stays at the best hit."""
import math
import os
import subprocess

import numpy as np
import pytest

from beluga_amd import build as mcl_build
from beluga_amd.amcl import Amcl, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam, OccupancyGrid, se2_from_xytheta

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_demo_hits_equal_the_python_facades(tmp_path):
    mcl_build.build()
    exe, lib_dir = str(tmp_path / "search_demo"), os.path.join(ROOT, "beluga_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "search_demo.cpp"), "-L", lib_dir, "-lbeluga_mcl", f"-Wl,-rpath,{lib_dir}", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    hits = [l.split()[1:] for l in lines if l.startswith("hit ")]
    estimate = [np.array(l.split()[1:], dtype=np.float64) for l in lines if l.startswith("estimate ")]
    assert 1 <= len(hits) <= 5 and len(estimate) == 1
    W, H = 64, 48
    cells = np.zeros((H, W), dtype=np.int8)
    cells[0, :] = cells[-1, :] = cells[:, 0] = cells[:, -1] = 100
    cells[30, [x for x in range(W) if x < 12 or x > 18]] = 100
    cells[:30, 40] = 100
    grid = OccupancyGrid(cells=cells, resolution=0.1, origin=se2_from_xytheta(-1.0, -1.0, 0.0))
    lf = LikelihoodFieldModelParam(max_obstacle_distance=2.0, max_laser_distance=100.0)
    scan = np.array([[3.0, 0.0], [0.0, 2.0], [-1.0, 0.0], [0.0, -1.0], [3.0, 1.0], [3.0, -1.0], [1.0, 2.0], [-1.0, 1.0]])
    f = Amcl(grid, DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05), lf, AmclParams(min_particles=300, max_particles=1500), seed=5)
    want = f.global_search(scan, headings=36, max_results=5)
    f.close()
    ros_hits = [l.split()[1:] for l in lines if l.startswith("ros_hit ")]
    for got in (hits, ros_hits):  # the plain facade's, and the ROS facade's over its laser scan type: the same points, the same hits
        assert [(int(h[0]), int(h[1])) for h in got] == [(h.cell, h.heading) for h in want]
        assert [float(h[2]) for h in got] == [h.score for h in want]
        assert [(float(h[3]), float(h[4])) for h in got] == [(h.pose[2], h.pose[3]) for h in want]
    best = want[0]
    assert math.hypot(estimate[0][0] - best.pose[2], estimate[0][1] - best.pose[3]) < 0.3
