"""The C++ facade's landmark fleet (AmclBatch over AmclLandmarkBatchSpec, tests/cpp/landmark_fleet_demo.cpp) against the Python
facade's AmclBatch.update_detections on the same inputs."""
import math
import os
import subprocess

import numpy as np
import pytest

from beluga_amd.amcl import (AmclBatch, AmclParams, LandmarkMap, LandmarkMapBoundaries, LandmarkModelParam, LandmarkPositionDetection,
                             se2_from_xytheta)

from test_gpu_landmark import MOTION

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_fleet_demo_matches_the_python_facade(tmp_path):
    lib_dir = os.path.join(ROOT, "beluga_amd", "lib")
    exe = tmp_path / "landmark_fleet_demo"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "landmark_fleet_demo.cpp"), "-L", lib_dir, "-lbeluga_mcl", f"-Wl,-rpath,{lib_dir}",
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    cpp = np.array([[float(v) for v in line.split()] for line in lines[:-1]])
    assert lines[-1].split() == ["launches", "12", "fused", "12"]  # (4 cycles: 3 launches and 3 members each)
    # the demo's scene: 12 landmarks on a circle of 5 m at heights 0.5 / 1.0 / 1.5, categories 0 .. 3; the robots stand at the origin
    entries = [((5.0 * math.cos(k * math.pi / 6), 5.0 * math.sin(k * math.pi / 6), 0.5 * (1 + k % 3)), k % 4) for k in range(12)]
    lm = LandmarkMap(LandmarkMapBoundaries((-6.0, -6.0, 0.0), (6.0, 6.0, 2.0)), [LandmarkPositionDetection(p, c) for p, c in entries])
    sensor = LandmarkModelParam(0.2, 0.1, 1e-3)
    batch = AmclBatch([dict(grid=lm, motion=MOTION, sensor=sensor, params=AmclParams(min_particles=n, max_particles=n), seed=7 + i,
                            landmark_small_cycle=True) for i, n in enumerate((2000, 1000, 500))])
    for member in batch.members:
        member.initialize((0.0, 0.0, 0.0), np.diag([0.04, 0.04, 0.01]))
    dets = [[LandmarkPositionDetection(p, c) for p, c in entries[i::2 + i]] for i in range(3)]
    rows = []
    for _ in range(4):
        for member in batch.members:
            member.force_update()
        for e in batch.update_detections([se2_from_xytheta(0, 0, 0)] * 3, dets):
            rows.append([e[0][2], e[0][3], math.atan2(e[0][1], e[0][0])])
    assert batch.counter("kernel_launches") == 12 and batch.counter("members_landmark_fused") == 12
    batch.close()
    np.testing.assert_allclose(cpp, np.array(rows), rtol=0, atol=1e-12)
