"""mcl_likelihoods* without a GPU: the symbols are declared and exported, the facade headers compile with the new members, and the
Python wrappers refuse wrong shapes and dtypes before any library call."""
import os
import re
import subprocess

import numpy as np
import pytest

from beluga_amd import amcl
from beluga_amd import build as mcl_build
from beluga_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mcl_likelihoods", "mcl_likelihoods_ndt_cells", "mcl_likelihoods_landmarks", "mcl_likelihoods_bearings", "mcl_likelihoods_device")


def test_entries_are_declared_exported_and_bound():
    mcl_build.build()
    lib = capi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "beluga_mcl.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bmcl_status\s+" + name + r"\s*\(", header), f"{name} is not declared in beluga_mcl.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in capi.exported_names()
        assert not name.startswith("mcl_batch_")


def test_facade_headers_compile_with_the_new_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text("""
#include "beluga_amd/ros_amcl.hpp"
using Points = std::vector<std::pair<double, double>>;
std::vector<double> (beluga_amd::Amcl::*points)(const std::vector<beluga_amd::SE2d>&, const Points&) = &beluga_amd::Amcl::likelihoods;
std::vector<double> (beluga_amd::Amcl::*landmarks)(const std::vector<beluga_amd::SE2d>&, const std::vector<beluga_amd::LandmarkPositionDetection>&) =
    &beluga_amd::Amcl::likelihoods;
std::vector<double> (beluga_amd::Amcl::*bearings)(const std::vector<beluga_amd::SE2d>&, const std::vector<beluga_amd::LandmarkBearingDetection>&) =
    &beluga_amd::Amcl::likelihoods;
int main() { return points && landmarks && bearings ? 0 : 1; }
""")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    demo = os.path.join(ROOT, "tests", "cpp", "likelihoods_demo.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), demo])


class NoLibrary:
    """Stands where the loaded library stands: any call through it is the failure this test looks for."""

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper reached the library ({name}) with arguments it has to refuse")


def detached(kind=0):
    f = amcl.Amcl.__new__(amcl.Amcl)
    f._lib, f._ctx, f._landmark_kind, f._owned = NoLibrary(), None, kind, False
    return f


GOOD_POSES = np.array([[1.0, 0.0, 0.5, 0.5], [0.0, 1.0, -0.5, 2.0]])
GOOD_POINTS = np.array([[1.0, 0.0], [0.0, 2.0], [3.0, 1.0]])


@pytest.mark.parametrize("poses, error", [
    (GOOD_POSES.astype(np.float32), TypeError), (np.ones((2, 4), dtype=np.int64), TypeError), (np.ones((2, 3)), ValueError),
    (np.ones(8), ValueError), (np.ones((2, 4, 1)), ValueError), (np.ones((2, 4), dtype=np.complex128), TypeError)])
def test_wrong_poses_are_refused_before_the_library(poses, error):
    for f, measurement in ((detached(), GOOD_POINTS), (detached(capi.MCL_SENSOR_LANDMARK), (np.ones((1, 3)), np.zeros(1, dtype=np.uint32)))):
        with pytest.raises(error):
            f.likelihoods(poses, measurement)
    with pytest.raises(error):
        detached().likelihoods_ndt_cells(poses, np.ones((1, 2)), np.ones((1, 4)))


@pytest.mark.parametrize("points, error", [(GOOD_POINTS.astype(np.float32), TypeError), (np.ones((3, 3)), ValueError), (np.ones(6), ValueError),
                                           (np.ones((3, 2), dtype=np.int32), TypeError)])
def test_wrong_points_are_refused_before_the_library(points, error):
    with pytest.raises(error):
        detached().likelihoods(GOOD_POSES, points)


def test_wrong_cells_and_detections_are_refused_before_the_library():
    f = detached()
    with pytest.raises(ValueError):
        f.likelihoods_ndt_cells(GOOD_POSES, np.ones((2, 2)), np.ones((3, 4)))
    with pytest.raises(ValueError):
        f.likelihoods_ndt_cells(GOOD_POSES, np.ones((2, 3)), np.ones((2, 4)))
    with pytest.raises(TypeError):
        f.likelihoods_ndt_cells(GOOD_POSES, np.ones((2, 2)), np.ones((2, 4), dtype=np.float32))
    for kind in (capi.MCL_SENSOR_LANDMARK, capi.MCL_SENSOR_BEARING):
        f = detached(kind)
        with pytest.raises(ValueError):
            f.likelihoods(GOOD_POSES, (np.ones((2, 3)), np.zeros(3, dtype=np.uint32)))
        with pytest.raises(ValueError):
            f.likelihoods(GOOD_POSES, (np.ones((2, 2)), np.zeros(2, dtype=np.uint32)))
        with pytest.raises(TypeError):
            f.likelihoods(GOOD_POSES, (np.ones((2, 3), dtype=np.float32), np.zeros(2, dtype=np.uint32)))
        with pytest.raises(TypeError):
            f.likelihoods(GOOD_POSES, (np.ones((2, 3)), np.zeros(2)))
        with pytest.raises(ValueError):
            f.likelihoods(GOOD_POSES, (np.ones((2, 3)), np.array([0, -1])))


def test_device_form_refuses_what_is_not_a_device_tensor_before_the_library():
    import torch

    f = detached()
    for poses in (GOOD_POSES, torch.from_numpy(GOOD_POSES)):  # a numpy array, a tensor in host memory
        with pytest.raises(TypeError):
            f.likelihoods_device(poses, GOOD_POINTS)
