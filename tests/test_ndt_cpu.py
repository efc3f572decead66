"""The 2D NDT sensor model without a GPU: the numpy restatement (tests/ndt_reference.py) pinned by the reference's own vectors
(beluga/test/beluga/sensor/test_ndt_model.cpp), the library's host-side measurement-cell fit (mcl_ndt_measurement_cells) against
it, the default parameters, argument checks that need no device, the fixture, and the C++ facade's NDT demo compiled with -Werror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from beluga_amd import build as mcl_build
from beluga_amd import capi, synth
from beluga_amd.amcl import default_ndt_params, load_ndt_map_npz, ndt_measurement_cells

import ndt_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DIAG = np.diag([0.5, 0.5])


def golden_map():  # test_ndt_model.cpp Likelihoood
    return ref.NdtMap([(0, 0), (1, 1)], [(0.5, 0.5), (1.5, 1.5)], [np.diag([0.5, 0.3]), np.diag([0.5, 0.5])], 1.0)


GOLDEN_LIKELIHOOD = [((0.5, 0.5), 1.3678794411714423), ((0.8, 0.5), 1.4307317817730123), ((0.5, 0.8), 1.4200370805919718),
                     ((1.5, 1.5), 1.3246524673583497), ((1.8, 1.5), 1.1859229670198237), ((1.5, 1.8), 1.1669230426687498)]
SENSOR_MODEL_POINTS = [(0.1, 0.2), (0.112, 0.22), (0.15, 0.23), (0.1, 0.24), (0.16, 0.25), (0.1, 0.26)]


def test_restatement_reproduces_the_reference_likelihood_vectors():
    m = golden_map()
    for mean, want in GOLDEN_LIKELIHOOD:
        assert ref.likelihood_at(m, mean, DIAG, minimum_likelihood=1e-6) == pytest.approx(want, rel=1e-14)
    for p in [(0.1, 0.1), (0.45, 0.45), (1.65, 0.65)]:  # MinLikelihood: an empty map gives the minimum
        assert ref.likelihood_at(ref.NdtMap([], [], [], 1.0), p, DIAG, minimum_likelihood=1e-6) == 1e-6


def sensor_model_map():  # test_ndt_model.cpp SensorModel (2D): the map is the fit of the measurement itself
    means, covs = ref.to_cells(SENSOR_MODEL_POINTS, 0.5)
    keys = [(int(m[0] / 0.5), int(m[1] / 0.5)) for m in means]
    return ref.NdtMap(keys, means, covs, 0.5), means, covs


def test_restatement_reproduces_the_reference_sensor_model_vector():
    m, means, covs = sensor_model_map()
    assert len(means) == 1
    st = lambda x, y, t=0.0: np.array([np.cos(t), np.sin(t), x, y])
    assert ref.weights(m, st(0, 0), means, covs)[0] == 2.0
    assert ref.weights(m, st(-10, -10), means, covs)[0] == 1.0
    assert ref.weights(m, st(0.1, 0.1), means, covs)[0] > 1.0


def test_restatement_fit_points_and_small_groups():
    mean, cov = ref.fit_points([(0.1, 0.2)] * 6)
    np.testing.assert_allclose(mean, (0.1, 0.2))
    assert np.all(np.diag(cov) == 1e-5)  # the clamp keeps the covariance away from zero
    mean, cov = ref.fit_points([(0.1, 0.2), (0.1, 0.9), (0.1, 0.2), (0.1, 0.9), (0.1, 0.2), (0.1, 0.2)])
    np.testing.assert_allclose(mean, (0.1, 0.433333), rtol=1e-6)
    assert cov[1, 1] > cov[0, 0]
    means, _ = ref.to_cells([(0.1, 0.2), (0.112, 0.22), (0.15, 0.23)], 0.5)  # ToCellsNotEnoughPointsInCell
    assert len(means) == 0


def test_turtlebot_fixture_has_the_reference_map():
    m = load_ndt_map_npz(os.path.join(GOLDEN, "turtlebot3_world_ndt.npz"))
    assert len(m.cells) == 30 and m.resolution == 1.0  # LoadFromHDF5HappyPath
    assert m.means.shape == (30, 2) and m.covariances.shape == (30, 2, 2)
    np.testing.assert_array_equal(np.floor(m.means / m.resolution).astype(np.int32), m.cells)  # keys are cell_near of the means
    np.testing.assert_array_equal(m.covariances, np.transpose(m.covariances, (0, 2, 1)))


def _cells_match(points, res):
    gm, gc = ndt_measurement_cells(points, res)
    wm, wc = ref.to_cells(points, res)
    assert gm.shape == wm.shape
    np.testing.assert_allclose(gm, wm, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(gc, wc, rtol=1e-10, atol=1e-15)
    return gm, gc


def test_measurement_cells_match_the_restatement():
    rng = np.random.Generator(np.random.PCG64(3))
    angles = synth.lidar_angles(1080, 270.0)
    pts = np.stack([np.cos(angles), np.sin(angles)], 1) * rng.uniform(0.5, 8.0, 1080)[:, None]
    gm, _ = _cells_match(pts, 1.0)
    assert len(gm) > 20
    _cells_match(pts, 0.25)


def test_measurement_cells_truncate_toward_zero_not_floor():
    # x in (-1, 0) and (0, 1) share key 0 under truncation (floor would split them): 3 + 3 points make one cell of 6
    pts = [(-0.3, 0.2), (-0.2, 0.3), (-0.1, 0.1), (0.1, 0.2), (0.2, 0.1), (0.3, 0.3)]
    gm, _ = _cells_match(pts, 1.0)
    assert len(gm) == 1
    np.testing.assert_allclose(gm[0], np.mean(pts, axis=0))
    # negative coordinates beyond one cell: key -1 holds (-1.5, ...) and not (-0.5, ...)
    pts2 = [(-1.5 - 0.01 * k, -2.5 + 0.02 * k) for k in range(5)] + [(-0.5, -0.5)] * 4
    gm, _ = _cells_match(pts2, 1.0)
    assert len(gm) == 1 and gm[0][0] < -1.0


def test_measurement_cells_groups_of_four_dropped_five_kept_and_variance_clamped():
    four = [(2.1 + 0.01 * k, 3.2) for k in range(4)]
    five = [(5.1, 5.2 + 0.01 * k) for k in range(5)]  # all at x = 5.1: variance in x is 0 -> clamped to 1e-5
    gm, gc = _cells_match(four + five, 1.0)
    assert len(gm) == 1
    np.testing.assert_allclose(gm[0], np.mean(five, axis=0))
    assert gc[0][0, 0] == 1e-5 and gc[0][1, 1] > 1e-5
    gm, _ = _cells_match(four, 1.0)
    assert len(gm) == 0
    gm, _ = _cells_match(np.zeros((0, 2)), 1.0)
    assert len(gm) == 0


def test_default_ndt_params_are_the_reference_struct():
    p = default_ndt_params()
    assert (p["minimum_likelihood"], p["d1"], p["d2"]) == (0.0, 1.0, 1.0)
    assert p["neighbors_kernel"] == ref.DEFAULT_KERNEL


def test_ndt_calls_validate_before_any_device_use():
    lib = capi.load()
    keys = np.zeros((1, 2), dtype=np.int32)
    m, c = np.zeros((1, 2)), np.eye(2).reshape(1, 4)
    st = lib.mcl_set_ndt_map(None, keys.ctypes.data_as(C.POINTER(C.c_int32)), m.ctypes.data_as(capi.c_double_p),
                             c.ctypes.data_as(capi.c_double_p), 1, 1.0, None)
    assert st == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.mcl_reweight_ndt_cells(None, None, None, 0) == capi.MCL_ERR_INVALID_ARGUMENT
    pts = np.zeros((6, 2))
    k = C.c_uint64(0)
    out = np.zeros(16)
    for res in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.mcl_ndt_measurement_cells(pts.ctypes.data_as(capi.c_double_p), 6, res, out.ctypes.data_as(capi.c_double_p),
                                             out.ctypes.data_as(capi.c_double_p), C.byref(k)) == capi.MCL_ERR_INVALID_ARGUMENT


def test_synthetic_ndt_map_keys_follow_cell_near():
    cells = synth.make_rooms_map(200, 200, seed=2, n_rooms=4)
    keys, means, covs = synth.make_ndt_map(cells, 0.05, 0.5, origin_xy=(-5.0, -5.0), seed=1)
    assert len(keys) > 50 and np.any(keys < 0)
    np.testing.assert_array_equal(np.floor(means / 0.5).astype(np.int32), keys)
    assert len({tuple(k) for k in keys}) == len(keys)
    assert np.all(covs[:, 0, 0] >= 1e-5) and np.all(covs[:, 1, 1] >= 1e-5)


def test_ndt_demo_compiles_against_the_facade(tmp_path):
    mcl_build.build()
    lib_dir = os.path.join(ROOT, "beluga_amd", "lib")
    exe = tmp_path / "ndt_demo"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ndt_demo.cpp"), "-L", lib_dir, "-lbeluga_mcl", f"-Wl,-rpath,{lib_dir}",
                           "-o", str(exe)])
    assert exe.exists()
