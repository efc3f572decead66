"""tests/cpp/cast_rays_demo.cpp: Amcl::cast_rays of the C++ facade on a likelihood-field and on a beam filter - ranges, hit cells and the
count of visited cells equal tests/raycast_reference.py and the Python facade's on the same grid, states and bearings, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import raycast_reference as rc
from beluga_amd import build as mcl_build
from beluga_amd.amcl import Amcl, AmclParams, BeamModelParam, DifferentialDriveModelParam, LikelihoodFieldModelParam, OccupancyGrid

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
MAX_RANGE = 2.5


def test_cpp_demo_rays_equal_the_reference_and_the_python_facades(tmp_path):
    mcl_build.build()
    exe, lib_dir = str(tmp_path / "cast_rays_demo"), os.path.join(ROOT, "beluga_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cast_rays_demo.cpp"), "-L", lib_dir, "-lbeluga_mcl", f"-Wl,-rpath,{lib_dir}", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.split("\n") if l]
    take = lambda word, dtype=np.float64: np.array([l[1:] for l in lines if l[0] == word], dtype=dtype)
    (W, H, resolution), origin = take("grid")[0], take("origin")[0]
    cells = take("row", np.int64).astype(np.int8)
    states, bearings, visited = take("state"), take("bearing"), take("visited", np.int64).reshape(-1)
    rays = [l[1:] for l in lines if l[0] == "ray"]
    assert cells.shape == (int(H), int(W)) and states.shape == (6, 4) and bearings.shape == (24, 2) and len(visited) == 2 and len(rays) == 2 * 6 * 24
    want = rc.cast_rays(cells, resolution, origin, states, bearings, MAX_RANGE)
    assert (want["hit_cells"][:5] >= 0).sum() > 60 and (want["hit_cells"][5] == -1).all() and (want["ranges"] < MAX_RANGE).any()
    grid = OccupancyGrid(cells=cells, resolution=float(resolution), origin=origin)
    sensors = (LikelihoodFieldModelParam(1.0, 2.0, 0.5, 0.5, 0.2), BeamModelParam(0.5, 0.5, 0.05, 0.05, 0.2, 0.1, MAX_RANGE))
    for k, sensor in enumerate(sensors):
        part = rays[144 * k:144 * (k + 1)]
        ranges = np.array([r[0] for r in part], dtype=np.float64).reshape(6, 24)
        hits = np.array([r[1] for r in part], dtype=np.int64).reshape(6, 24)
        assert np.array_equal(ranges.view(np.uint64), want["ranges"].view(np.uint64)) and np.array_equal(hits, want["hit_cells"]), k
        assert visited[k] == want["cells_visited"], k
        f = Amcl(grid, MOTION, sensor, AmclParams(min_particles=100, max_particles=100), seed=7)
        got = f.cast_rays(states, bearings=bearings, max_range=MAX_RANGE, hit_cells=True, cells_visited=True)
        f.close()
        assert np.array_equal(got[0].view(np.uint64), ranges.view(np.uint64)) and np.array_equal(got[1], hits) and got[2] == visited[k]
