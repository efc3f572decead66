"""tests/cpp/likelihoods_demo.cpp: Amcl::likelihoods of the C++ facade on a landmark and on a bearing filter - its scores equal the
Python facade's on the same states, map and detections, bit for bit (both are the same call of the C ABI), and its best candidate is the
best of those scores."""
import os
import subprocess

import numpy as np
import pytest

from beluga_amd import build as mcl_build
from beluga_amd.amcl import (Amcl, AmclParams, BearingModelParam, DifferentialDriveModelParam, LandmarkMap, LandmarkMapBoundaries,
                             LandmarkModelParam, LandmarkPositionDetection)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
HEIGHT = 0.5


def test_cpp_demo_scores_equal_the_python_facades(tmp_path):
    mcl_build.build()
    exe, lib_dir = str(tmp_path / "likelihoods_demo"), os.path.join(ROOT, "beluga_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "likelihoods_demo.cpp"), "-L", lib_dir, "-lbeluga_mcl", f"-Wl,-rpath,{lib_dir}", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    landmarks = [l.split()[1:] for l in lines if l.startswith("landmark ")]
    best = [np.array(l.split()[1:], dtype=np.float64) for l in lines if l.startswith("best ")]
    rows = np.array([l.split() for l in lines if l and l[0] in "-0123456789"], dtype=np.float64)
    assert len(landmarks) == 12 and len(best) == 2 and rows.shape == (2 * 75, 5)
    positions = np.array([l[:3] for l in landmarks], dtype=np.float64)
    categories = np.array([l[3] for l in landmarks], dtype=np.uint32)
    box = LandmarkMapBoundaries((-6.0, -6.0, 0.0), (6.0, 6.0, 2.0))
    landmark_map = LandmarkMap(box, [LandmarkPositionDetection(tuple(p), int(c)) for p, c in zip(positions, categories)])
    seen, seen_cat = positions[::2], categories[::2]
    sensors = (LandmarkModelParam(sigma_range=0.2, sigma_bearing=0.1, random_prob=1e-3),
               BearingModelParam(sigma_bearing=0.1, sensor_pose_in_robot=(0.0, 0.0, 0.0, 1.0, 0.0, 0.0, HEIGHT)))
    for k, sensor in enumerate(sensors):
        part = rows[75 * k:75 * (k + 1)]
        vectors = seen - (np.array([0.0, 0.0, HEIGHT]) if k else 0.0)
        f = Amcl(landmark_map, MOTION, sensor, AmclParams(min_particles=500, max_particles=500), seed=7)
        got = f.likelihoods(np.ascontiguousarray(part[:, :4]), (np.ascontiguousarray(vectors), seen_cat))
        f.close()
        assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(part[:, 4]).view(np.uint64)), k
        top = part[np.argmax(part[:, 4])]
        assert best[k][0] == top[2] and best[k][1] == top[3]
        assert got.max() > 100 * np.median(got)  # (the lattice does tell the candidates apart)
