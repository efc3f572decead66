"""tests/cpp/range_table_demo.cpp: the range table of the beam model through the C++ facade - build_range_table, range_table_info,
range_table_bearings, range_table, drop_range_table - on a small room: the table equals tests/range_table_reference.py fed with the
bearings the program printed, the likelihoods over it are the Python facade's bits and the reference's within the beam bar, and after the
drop the likelihoods are the exact walk's bits."""
import os
import subprocess

import numpy as np
import pytest

import range_table_reference as rt
from beluga_amd import build as mcl_build
from beluga_amd.amcl import Amcl, AmclParams, BeamModelParam, DifferentialDriveModelParam, OccupancyGrid

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
MAX_RANGE = 2.5


def test_cpp_demo_table_equals_the_reference_and_the_python_facade(tmp_path):
    mcl_build.build()
    exe, lib_dir = str(tmp_path / "range_table_demo"), os.path.join(ROOT, "beluga_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "range_table_demo.cpp"), "-L", lib_dir, "-lbeluga_mcl", f"-Wl,-rpath,{lib_dir}", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = [l.split() for l in out.stdout.split("\n") if l]
    take = lambda word, dtype=np.float64: np.array([l[1:] for l in lines if l[0] == word], dtype=dtype)
    (W, H, resolution), origin = take("grid")[0], take("origin")[0]
    W, H, A = int(W), int(H), int(take("angles", np.int64)[0, 0])
    cells = take("row", np.int64).astype(np.int8)
    bearings, states, points = take("bearing"), take("state"), take("point")
    entries = take("entry", np.int64)
    assert cells.shape == (H, W) and bearings.shape == (A, 2) and states.shape == (6, 4) and points.shape == (16, 2) and len(entries) == W * H * A
    assert np.array_equal(entries[:, 0] * A + entries[:, 1], np.arange(W * H * A))
    assert np.max(np.abs(bearings - rt.bearings_of(A))) <= 1e-15
    table = entries[:, 2].reshape(H, W, A)
    want = rt.table(cells, resolution, MAX_RANGE, bearings)
    assert np.array_equal(table, want) and (want == rt.NO_HIT).any() and ((want != rt.NO_HIT) & (want > 0)).any()
    params = (0.5, 0.5, 0.05, 0.05, 0.2, 0.1, MAX_RANGE)  # (the facade's defaults but for the range)
    case = dict(cells=cells, resolution=float(resolution), origin=origin, states=states, points=points, params=params)
    r = rt.weights(case, want, A)
    over_table, exact = take("table_likelihood").reshape(-1), take("exact_likelihood").reshape(-1)
    assert r["margin"].min() >= 1e-6  # (on the reference alone: the demo's fixed poses and beams stay clear of the bin edges)
    assert np.max(np.abs(over_table - r["weights"]) / r["weights"]) <= 1e-10
    f = Amcl(OccupancyGrid(cells=cells, resolution=float(resolution), origin=origin), MOTION, BeamModelParam(*params),
             AmclParams(min_particles=100, max_particles=100), seed=7)
    try:
        assert np.array_equal(f.likelihoods(states, points).view(np.uint64), exact.view(np.uint64))
        f.build_range_table(A)
        assert np.array_equal(f.range_table().astype(np.int64), table) and np.array_equal(f.range_table_bearings().view(np.uint64), bearings.view(np.uint64))
        assert np.array_equal(f.likelihoods(states, points).view(np.uint64), over_table.view(np.uint64))
    finally:
        f.close()
