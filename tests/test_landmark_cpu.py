"""The landmark and bearing sensor models without a GPU: the numpy restatement (tests/landmark_reference.py) pinned by the reference's
own cases (beluga/test/beluga/sensor/test_landmark_sensor_model.cpp, test_bearing_sensor_model.cpp) within their tolerances and to
1e-12 against the closed forms they stand for, the tie rule, the default parameters, the checks that need no device, and the C++
facade's landmark demo compiled with -Werror."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from beluga_amd import build as mcl_build
from beluga_amd import capi
from beluga_amd.amcl import (BearingModelParam, LandmarkMap, LandmarkMapBoundaries, LandmarkModelParam, LandmarkPositionDetection,
                             default_bearing_params, default_landmark_params)

import landmark_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = ((-10.0, -10.0, 0.0), (10.0, 10.0, 0.0))  # default_map_boundaries of both reference tests
POSE = np.array([math.cos(-math.pi / 2), math.sin(-math.pi / 2), 1.0, -1.0])  # get_robot_pose_in_world<SE2d>
LANDMARK = dict(sigma_range=1.0, sigma_bearing=math.pi / 2, random_prob=1e-4)
BEARING = dict(sigma_bearing=math.pi / 4, sensor_pose_in_robot=(0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0))
ONE_STD = math.exp(-0.5)


def lmap(entries):
    return ref.LandmarkMap([e[0] for e in entries], [e[1] for e in entries], BOX)


def landmark_weight(entries, detections, **kw):
    w, _ = ref.landmark_weights(lmap(entries), POSE, [d[0] for d in detections], [d[1] for d in detections], **{**LANDMARK, **kw})
    return float(w[0])


def bearing_weight(entries, detections, **kw):
    w, _ = ref.bearing_weights(lmap(entries), POSE, [d[0] for d in detections], [d[1] for d in detections], **{**BEARING, **kw})
    return float(w[0])


# (map, detections, the reference test's expectation, its tolerance, the closed form)
P = LANDMARK["random_prob"]
LANDMARK_CASES = {
    "BullsEyeDetection": ([((3, -2, 0), 0)], [((1, 2, 0), 0)], 1.0, 1e-2, 1.0 + P),
    "MapUpdate_empty": ([], [((1, 2, 0), 0)], 0.0, 1e-2, P),
    "MapUpdate_updated": ([((3, -2, 0), 0)], [((1, 2, 0), 0)], 1.0, 1e-2, 1.0 + P),
    "MultipleBullsEyeDetections": ([((1, -2, 0), 0), ((1, -0, 0), 1), ((2, -1, 0), 2), ((0, -1, 0), 3)],
                                   [((1, 0, 0), 0), ((-1, 0, 0), 1), ((0, 1, 0), 2), ((0, -1, 0), 3)], 1.0, 1e-2, (1.0 + P) ** 4),
    "OneStdInRange_baseline": ([((1, -11, 0), 0)], [((10, 0, 0), 0)], 1.0, 1e-2, 1.0 + P),
    "OneStdInRange_default": ([((1, -11, 0), 0)], [((9, 0, 0), 0)], 0.6, 1e-2, ONE_STD + P),
    "OneStdInRange_excess": ([((1, -11, 0), 0)], [((11, 0, 0), 0)], 0.6, 1e-2, ONE_STD + P),
    "OneStdInBearing_default": ([((1, -11, 0), 0)], [((0, 10, 0), 0)], 0.6, 1e-2, ONE_STD + P),
    "OneStdInBearing_excess": ([((1, -11, 0), 0)], [((0, -10, 0), 0)], 0.6, 1e-2, ONE_STD + P),
    "NoSuchLandmark": ([((0, 1, 0), 99)], [((0, 2, 0), 88)], P, 1e-6, P),
    "FalsePositiveLandmark": ([((0, 1, 0), 0)], [((0, 10, 0), 0)], P, 1e-6, None),
}
BEARING_CASES = {
    "BullsEyeDetection": ([((1, -2, 1), 0)], [((1, 0, 0), 0)], 1.0, 1e-2, 1.0),
    "MapUpdate_empty": ([], [((1, 0, 0), 0)], 0.0, 1e-2, 0.0),
    "MapUpdate_updated": ([((1, -2, 1), 0)], [((1, 0, 0), 0)], 1.0, 1e-2, 1.0),
    "MultipleBullsEyeDetections": ([((1, -2, 0), 0), ((1, -2, 1), 1), ((1, -2, 2), 2)],
                                   [((1, 0, -1), 0), ((1, 0, 0), 1), ((1, 0, 1), 2)], 1.0, 1e-2, 1.0),
    "OneStdInBearing_left": ([((1, -2, 1), 0)], [((1, 1, 0), 0)], 0.6, 1e-2, ONE_STD),
    "OneStdInBearing_right": ([((1, -2, 1), 0)], [((1, -1, 0), 0)], 0.6, 1e-2, ONE_STD),
    "OneStdInBearing_up": ([((1, -2, 1), 0)], [((1, 0, 1), 0)], 0.6, 1e-2, ONE_STD),
    "OneStdInBearing_down": ([((1, -2, 1), 0)], [((1, 0, -1), 0)], 0.6, 1e-2, ONE_STD),
    "NoSuchLandmark": ([((1, -1, 1), 0)], [((1, 0, 0), 99)], 0.0, 1e-2, 0.0),
}


@pytest.mark.parametrize("name", sorted(LANDMARK_CASES))
def test_restatement_reproduces_the_reference_landmark_cases(name):
    entries, detections, expected, tolerance, closed = LANDMARK_CASES[name]
    got = landmark_weight(entries, detections)
    assert abs(got - expected) <= tolerance
    if closed is not None:
        assert got == pytest.approx(closed, rel=1e-12, abs=1e-300)


@pytest.mark.parametrize("name", sorted(BEARING_CASES))
def test_restatement_reproduces_the_reference_bearing_cases(name):
    entries, detections, expected, tolerance, closed = BEARING_CASES[name]
    got = bearing_weight(entries, detections)
    assert abs(got - expected) <= tolerance
    assert got == pytest.approx(closed, rel=1e-12, abs=0.0)


def test_no_detections_leave_the_weight_unchanged_and_the_product_runs_in_blocks_of_four():
    assert landmark_weight([((1, 1, 0), 0)], []) == 1.0
    assert bearing_weight([((1, 1, 0), 0)], []) == 1.0
    rng = np.random.Generator(np.random.PCG64(1))
    t = rng.uniform(0.1, 0.9, (9, 1))
    want = 1.0 * ((t[0] * t[1]) * (t[2] * t[3]))
    want = want * ((t[4] * t[5]) * (t[6] * t[7]))
    want = want * t[8]
    assert ref.transform_reduce_product(t)[0] == want[0]


# Exactly tied candidates: identity heading, coordinates that are exact in binary, so both distances (dot products) are equal to the bit.
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0])
TIE_LANDMARKS = [((2.0, 1.0, 0.0), 7), ((2.0, -1.0, 0.0), 7)]  # both sqrt(2) away from the detection at (1, 0, 0) ...
TIE_DETECTION = [((1.0, 0.0, 0.0), 7)]                         # ... and on either side of it


def tie_weights(first_to_second):
    entries = TIE_LANDMARKS if first_to_second else TIE_LANDMARKS[::-1]
    m = ref.LandmarkMap([e[0] for e in entries], [e[1] for e in entries], BOX)
    det, cat = [d[0] for d in TIE_DETECTION], [d[1] for d in TIE_DETECTION]
    lw, lg = ref.landmark_weights(m, IDENTITY, det, cat, sigma_range=0.5, sigma_bearing=0.25, random_prob=1e-4)
    # bearing: the detection (1, 0, 1) against landmarks at (2, 0, 0) and (0, 0, 2) seen from the origin - dot products 1 and 1
    b = ref.LandmarkMap([(2.0, 0.0, 0.0), (0.0, 0.0, 2.0)] if first_to_second else [(0.0, 0.0, 2.0), (2.0, 0.0, 0.0)], [7, 7], BOX)
    bw, bg = ref.bearing_weights(b, IDENTITY, [(1.0, 0.0, 1.0)], [7], sigma_bearing=0.5)
    return float(lw[0]), float(lg[0, 0]), float(bw[0]), float(bg[0, 0])


def test_tied_candidates_pick_the_first_in_map_order():
    lw, lg, bw, bg = tie_weights(True)
    assert lg == 0.0 and bg == 0.0  # tied to the bit
    # landmark: both candidates are sqrt(2) from the detection; the first, (2, 1, 0), is at range sqrt(5) and atan2(1, 2) off the detection
    want = math.exp(-(1.0 - math.sqrt(5.0)) ** 2 / 0.5) * math.exp(-math.atan2(1.0, 2.0) ** 2 / 0.125) + 1e-4
    assert lw == pytest.approx(want, rel=1e-12)
    # both orders give the same value here (the candidates mirror each other), so the pick itself is pinned with an asymmetric pair:
    m = ref.LandmarkMap([(3.0, 0.0, 0.0), (1.0, 2.0, 0.0)], [7, 7], BOX)  # 2 m beyond the detection / 2 m beside it
    a, g = ref.landmark_weights(m, IDENTITY, [(1.0, 0.0, 0.0)], [7], sigma_range=0.5, sigma_bearing=0.25, random_prob=1e-4)
    assert g[0, 0] == 0.0
    assert a[0] == pytest.approx(math.exp(-(1.0 - 3.0) ** 2 / 0.5) + 1e-4, rel=1e-12)  # the first: on the detection's bearing, 2 m farther
    m = ref.LandmarkMap([(1.0, 2.0, 0.0), (3.0, 0.0, 0.0)], [7, 7], BOX)
    b, _ = ref.landmark_weights(m, IDENTITY, [(1.0, 0.0, 0.0)], [7], sigma_range=0.5, sigma_bearing=0.25, random_prob=1e-4)
    assert b[0] == pytest.approx(math.exp(-(1.0 - math.sqrt(5.0)) ** 2 / 0.5) * math.exp(-math.atan2(2.0, 1.0) ** 2 / 0.125) + 1e-4, rel=1e-12)
    assert a[0] != b[0]
    # bearing: the first of the two, (2, 0, 0), is pi / 4 off the detection (1, 0, 1); so is the other - the order shows in the pick only
    assert bw == pytest.approx(math.exp(-(math.pi / 4) ** 2 / 0.5), rel=1e-12)


def test_duplicate_landmarks_do_not_count_as_a_runner_up():
    m = ref.LandmarkMap([(2.0, 1.0, 0.0), (2.0, 1.0, 0.0), (5.0, 5.0, 0.0)], [1, 1, 1], BOX)
    _, g = ref.landmark_weights(m, IDENTITY, [(2.0, 1.0, 0.0)], [1])
    assert g[0, 0] == 1.0  # the runner-up is (5, 5, 0), not the duplicate


def test_landmark_map_constructors_and_limits():
    entries = [LandmarkPositionDetection((1.0, -2.0, 0.5), 3), LandmarkPositionDetection((-4.0, 6.0, 2.0), 1)]
    m = LandmarkMap(entries)
    np.testing.assert_array_equal(m.map_limits().min, (-4.0, -2.0, 0.5))
    np.testing.assert_array_equal(m.map_limits().max, (1.0, 6.0, 2.0))
    m = LandmarkMap(LandmarkMapBoundaries(*BOX), entries)
    assert tuple(m.map_limits().min) == BOX[0] and tuple(m.map_limits().max) == BOX[1]
    np.testing.assert_array_equal(m.categories, [3, 1])
    assert LandmarkMap(LandmarkMapBoundaries(*BOX), []).positions.shape == (0, 3)
    r = ref.LandmarkMap([e.detection_position_in_robot for e in entries], [e.category for e in entries])
    np.testing.assert_array_equal(r.map_limits()[0], (-4.0, -2.0, 0.5))


def test_defaults_are_the_reference_structs():
    assert default_landmark_params() == {"sigma_range": 1.0, "sigma_bearing": 1.0, "random_prob": 1e-4}
    assert default_bearing_params() == {"sigma_bearing": 1.0, "sensor_pose_in_robot": (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)}
    assert LandmarkModelParam() == LandmarkModelParam(1.0, 1.0, 1e-4)
    assert BearingModelParam() == BearingModelParam(1.0, (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0))
    assert (capi.MCL_SENSOR_LANDMARK, capi.MCL_SENSOR_BEARING) == (4, 5)


def test_landmark_calls_validate_before_any_device_use():
    lib = capi.load()
    pos = np.zeros((1, 3))
    cat = np.zeros(1, dtype=np.uint32)
    ctrl = np.array([1.0, 0.0, 0.0, 0.0])
    dp, up = capi.c_double_p, capi.c_u32_p
    assert lib.mcl_set_landmark_map(None, pos.ctypes.data_as(dp), cat.ctypes.data_as(up), 1, None, None) == capi.MCL_ERR_INVALID_ARGUMENT
    for fn in (lib.mcl_reweight_landmarks, lib.mcl_reweight_bearings):
        assert fn(None, pos.ctypes.data_as(dp), cat.ctypes.data_as(up), 1) == capi.MCL_ERR_INVALID_ARGUMENT
    for fn in (lib.mcl_update_landmarks, lib.mcl_update_bearings):
        assert fn(None, ctrl.ctypes.data_as(dp), pos.ctypes.data_as(dp), cat.ctypes.data_as(up), 1, None, None) == capi.MCL_ERR_INVALID_ARGUMENT
    lib.mcl_default_landmark_params(None)  # (a null struct is ignored)
    lib.mcl_default_bearing_params(None)
    # an unknown sensor kind is refused at creation, before the device is looked for
    cfg = capi.Config()
    lib.mcl_default_config(C.byref(cfg))
    cfg.sensor_kind = 6
    ctx = capi._ctx()
    assert lib.mcl_create(C.byref(cfg), C.byref(ctx)) == capi.MCL_ERR_INVALID_ARGUMENT


def test_landmark_demo_compiles_against_the_facade(tmp_path):
    mcl_build.build()
    lib_dir = os.path.join(ROOT, "beluga_amd", "lib")
    exe = tmp_path / "landmark_demo"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "landmark_demo.cpp"), "-L", lib_dir, "-lbeluga_mcl", f"-Wl,-rpath,{lib_dir}",
                           "-o", str(exe)])
    assert exe.exists()
