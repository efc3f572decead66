"""The host passes of the NDT, landmark and bearing sensor models (beluga_amd/csrc/ndt_host.cpp, landmark_host.cpp) on the CPU: a
plain g++ compiles them with a short driver that reads its arguments from a binary file, calls one of the functions and writes what
it returned.  What a context would upload - the index grid and the cell records of an NDT map, the grouped landmarks with their
category ranges, the detection records - is checked here against the fixtures and the numpy restatements (tests/ndt_reference.py,
tests/landmark_reference.py), with the refusals in the library's own words, without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from beluga_amd import capi
from beluga_amd.amcl import load_ndt_map_npz, ndt_measurement_cells

import landmark_reference as lref
import ndt_reference as nref
from test_ndt_build_cpu import hand_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

DRIVER = r"""
// driver <what> <in> <out>: both files are 8-byte words, integers as int64 and reals as double.  Every answer but fit's starts with the
// status and the message (its length, then its bytes padded to whole words).
//   fit      in: resolution, B, points[2B]                                   out: the records
//   ndtmap   in: resolution, n, P (0: no params), [minimum_likelihood, d1, d2, num_offsets, offsets[64]], cells[2n], means[2n], covs[4n]
//            out: reach, grid_x0, grid_y0, gw, gh, num_offsets, the grid [gw * gh], the records [6n]
//   lmmap    in: kind, n, B (0: no boundaries), P (0: no params), params[8], positions[3n], categories[n], boundaries[6]
//            out: den_range, den_bearing, random_prob, Rs[9], ts[3], lo[3], hi[3], the landmarks [4n], R, (category, first, count)[R]
//   records  in: kind, n, R (-1: no map), (category, first, count)[R], xyz[3n], categories[n]
//            out: the records [10n]
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "landmark_host.h"
#include "ndt_host.h"

using namespace mcl;

static std::vector<long long> in;
static size_t at = 0;
static std::FILE* out = nullptr;
static long long word() { return in[at++]; }
static double real() {
  double v;
  std::memcpy(&v, &in[at++], sizeof v);
  return v;
}
static std::vector<double> reals(size_t n) {
  std::vector<double> v(n);
  for (double& x : v) x = real();
  return v;
}
static void put(long long v) { std::fwrite(&v, sizeof v, 1, out); }
static void put(double v) { std::fwrite(&v, sizeof v, 1, out); }
static void put(const double* v, size_t n) { std::fwrite(v, sizeof(double), n, out); }
static void put_status(mcl_status s, const std::string& message) {
  put(static_cast<long long>(s));
  put(static_cast<long long>(message.size()));
  std::string padded = message;
  padded.resize((message.size() + 7) / 8 * 8, '\0');
  std::fwrite(padded.data(), 1, padded.size(), out);
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 2;
  std::fseek(f, 0, SEEK_END);
  in.resize(static_cast<size_t>(std::ftell(f)) / sizeof(long long));
  std::fseek(f, 0, SEEK_SET);
  if (std::fread(in.data(), sizeof(long long), in.size(), f) != in.size()) return 2;
  std::fclose(f);
  out = std::fopen(argv[3], "wb");
  if (!out) return 2;
  const std::string what = argv[1];
  std::string error;
  if (what == "fit") {
    const double resolution = real();
    const size_t B = static_cast<size_t>(word());
    const std::vector<double> pts = reals(2 * B);
    std::vector<double> recs;
    ndt_fit_cells(pts.data(), B, resolution, recs);
    put(recs.data(), recs.size());
  } else if (what == "ndtmap") {
    const double resolution = real();
    const size_t n = static_cast<size_t>(word());
    mcl_ndt_params prm{};
    const bool have_params = word() != 0;
    if (have_params) {
      prm.minimum_likelihood = real(), prm.d1 = real(), prm.d2 = real();
      prm.num_offsets = static_cast<uint32_t>(word());
      for (int k = 0; k < 2 * MCL_NDT_MAX_OFFSETS; ++k) prm.offsets[k] = static_cast<int32_t>(word());
    }
    std::vector<int32_t> cells(2 * n);
    for (int32_t& c : cells) c = static_cast<int32_t>(word());
    const std::vector<double> means = reals(2 * n), covs = reals(4 * n);
    NdtMapLayout map;
    const mcl_status s = ndt_layout_map(cells.data(), means.data(), covs.data(), n, resolution, have_params ? &prm : nullptr, &map, &error);
    put_status(s, error);
    if (s == MCL_OK) {
      const NdtGridShape& g = map.shape;
      for (long long v : {static_cast<long long>(g.reach), static_cast<long long>(g.grid_x0), static_cast<long long>(g.grid_y0),
                          static_cast<long long>(g.gw), static_cast<long long>(g.gh), static_cast<long long>(map.params.num_offsets)})
        put(v);
      for (const int32_t v : map.grid) put(static_cast<long long>(v));
      put(map.records.data(), map.records.size());
    }
  } else if (what == "lmmap") {
    const int32_t kind = static_cast<int32_t>(word());
    const size_t n = static_cast<size_t>(word());
    const bool have_boundaries = word() != 0, have_params = word() != 0;
    const std::vector<double> p = reals(8);
    mcl_landmark_params lp{p[0], p[1], p[2]};
    mcl_bearing_params bp{p[0], {p[1], p[2], p[3], p[4], p[5], p[6], p[7]}};
    const std::vector<double> positions = reals(3 * n);
    std::vector<uint32_t> categories(n);
    for (uint32_t& c : categories) c = static_cast<uint32_t>(word());
    const std::vector<double> boundaries = reals(6);
    const void* params = !have_params ? nullptr : kind == MCL_SENSOR_LANDMARK ? static_cast<const void*>(&lp) : static_cast<const void*>(&bp);
    LandmarkMapLayout map;
    const mcl_status s = landmark_layout_map(kind, n ? positions.data() : nullptr, n ? categories.data() : nullptr, n,
                                             have_boundaries ? boundaries.data() : nullptr, params, &map, &error);
    put_status(s, error);
    if (s == MCL_OK) {
      put(map.den_range), put(map.den_bearing), put(map.random_prob);
      put(map.Rs, 9), put(map.ts, 3), put(map.lo, 3), put(map.hi, 3);
      put(map.landmarks.data(), map.landmarks.size());
      put(static_cast<long long>(map.ranges.size()));
      for (const auto& r : map.ranges) put(static_cast<long long>(r.first)), put(static_cast<long long>(r.second.first)), put(static_cast<long long>(r.second.second));
    }
  } else if (what == "records") {
    const int32_t kind = static_cast<int32_t>(word());
    const size_t n = static_cast<size_t>(word());
    const long long R = word();
    LandmarkRanges ranges;
    for (long long r = 0; r < R; ++r) {
      const uint32_t category = static_cast<uint32_t>(word()), first = static_cast<uint32_t>(word()), count = static_cast<uint32_t>(word());
      ranges[category] = {first, count};
    }
    const std::vector<double> xyz = reals(3 * n);
    std::vector<uint32_t> categories(n);
    for (uint32_t& c : categories) c = static_cast<uint32_t>(word());
    std::vector<double> recs;
    const mcl_status s = landmark_records("driver", kind, xyz.data(), categories.data(), n, R < 0 ? nullptr : &ranges, recs, &error);
    put_status(s, error);
    if (s == MCL_OK) put(recs.data(), recs.size());
  } else {
    return 2;
  }
  std::fclose(out);
  return at == in.size() ? 0 : 3;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("sensor_host")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    csrc = os.path.join(ROOT, "beluga_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", csrc, "-I", os.path.join(ROOT, "include"), str(src),
                           os.path.join(csrc, "ndt_host.cpp"), os.path.join(csrc, "landmark_host.cpp"), "-o", str(exe)])
    return str(exe), d


def _i(*values):
    return np.asarray(values, dtype=np.int64).reshape(-1)


def _f(*values):
    return np.asarray(values, dtype=np.float64).reshape(-1).view(np.int64)


def _call(driver, what, *parts):
    exe, d = driver
    np.concatenate(parts).tofile(str(d / "in.bin"))
    subprocess.check_call([exe, what, str(d / "in.bin"), str(d / "out.bin")])
    return np.fromfile(str(d / "out.bin"), dtype=np.int64)


def _status(words):
    """(status, message, the words behind them)"""
    size = int(words[1])
    padded = (size + 7) // 8
    return int(words[0]), words[2:2 + padded].tobytes()[:size].decode(), words[2 + padded:]


# ---- NDT: the fit of the measurement cells ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_ndt_fit_is_the_librarys_bit_for_bit_and_matches_the_restatement(driver, name):
    pts, res, keys = hand_cases()[name]
    recs = _call(driver, "fit", _f(res), _i(len(pts)), _f(pts)).view(np.float64).reshape(-1, 6)
    assert len(recs) == len(keys)
    means, covs = recs[:, :2], np.stack([recs[:, 2], recs[:, 3], recs[:, 3], recs[:, 4]], 1).reshape(-1, 2, 2)
    assert np.all(recs[:, 5] == 0.0)
    lib_means, lib_covs = ndt_measurement_cells(pts, res)  # the same code in the built library: other flags would show here
    assert np.array_equal(means, lib_means) and np.array_equal(covs, lib_covs)
    want_means, want_covs = nref.to_cells(pts, res)  # test_ndt_cpu.py's bounds: numpy adds a cell's points in another order
    np.testing.assert_allclose(means, want_means, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(covs, want_covs, rtol=1e-10, atol=1e-15)


# ---- NDT: the map's layout ----------------------------------------------------------------------------------------------------------

def _ndt_params(minimum_likelihood=0.0, d1=1.0, d2=1.0, offsets=nref.DEFAULT_KERNEL, num_offsets=None):
    flat = np.zeros(64, dtype=np.int64)
    flat[:2 * len(offsets)] = np.asarray(offsets, dtype=np.int64).reshape(-1)
    return [_i(1), _f(minimum_likelihood, d1, d2), _i(len(offsets) if num_offsets is None else num_offsets), flat]


def _ndt_map(driver, cells, means, covs, resolution=1.0, params=None):
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
    words = _call(driver, "ndtmap", _f(resolution), _i(len(cells)), *(params if params is not None else [_i(0)]), _i(cells), _f(means), _f(covs))
    status, message, rest = _status(words)
    if status != capi.MCL_OK:
        assert len(rest) == 0
        return status, message, None
    reach, gx0, gy0, gw, gh, num_offsets = (int(v) for v in rest[:6])
    grid = rest[6:6 + gw * gh].reshape(gh, gw)
    recs = rest[6 + gw * gh:].view(np.float64).reshape(len(cells), 6)
    return status, message, dict(reach=reach, grid_x0=gx0, grid_y0=gy0, gw=gw, gh=gh, num_offsets=num_offsets, grid=grid, records=recs)


def test_ndt_map_layout_of_the_turtlebot_map(driver):
    m = load_ndt_map_npz(os.path.join(GOLDEN, "turtlebot3_world_ndt.npz"))
    status, message, got = _ndt_map(driver, m.cells, m.means, m.covariances)
    assert (status, message) == (capi.MCL_OK, "") and len(m.cells) == 30
    assert got["reach"] == 1 and got["num_offsets"] == 9  # the default kernel
    x, y = m.cells[:, 0].astype(np.int64), m.cells[:, 1].astype(np.int64)
    assert got["gw"] == (x.max() - x.min() + 1) + 4 * got["reach"] and got["gh"] == (y.max() - y.min() + 1) + 4 * got["reach"]
    assert (got["grid_x0"], got["grid_y0"]) == (x.min() - 2 * got["reach"], y.min() - 2 * got["reach"])
    want = np.full((got["gh"], got["gw"]), -1, dtype=np.int64)
    want[y - got["grid_y0"], x - got["grid_x0"]] = np.arange(30)
    assert np.array_equal(got["grid"], want)  # every key finds its cell, every other entry is -1
    c = m.covariances
    assert np.array_equal(got["records"], np.stack([m.means[:, 0], m.means[:, 1], c[:, 0, 0], c[:, 0, 1], c[:, 1, 1], np.zeros(30)], 1))


TWO_CELLS = ([(0, 0), (1, 2)], [(0.5, 0.5), (1.5, 2.5)], [np.diag([0.5, 0.3]), np.diag([0.4, 0.6])])


def _two_cells(cells=None, means=None, covs=None):
    return (TWO_CELLS[0] if cells is None else cells, np.array(TWO_CELLS[1] if means is None else means), np.array(TWO_CELLS[2] if covs is None else covs))


NDT_REFUSALS = {
    "duplicate_key": (dict(cells=[(3, -4), (3, -4)]), None, capi.MCL_ERR_INVALID_ARGUMENT, "mcl_set_ndt_map: duplicate key (3, -4)"),
    "asymmetric": (dict(covs=[np.diag([0.5, 0.3]), [[0.4, 0.1], [0.1000001, 0.6]]]), None, capi.MCL_ERR_INVALID_ARGUMENT,
                   "mcl_set_ndt_map: the covariance of cell 1 is not symmetric"),
    "mean_not_finite": (dict(means=[(0.5, float("inf")), (1.5, 2.5)]), None, capi.MCL_ERR_INVALID_ARGUMENT,
                        "mcl_set_ndt_map: cell 0 has a value that is not finite"),
    "offset_65": ({}, dict(offsets=((0, 0), (65, 0))), capi.MCL_ERR_INVALID_ARGUMENT, "mcl_set_ndt_map: kernel offsets are limited to 64 cells"),
    "no_offsets": ({}, dict(offsets=(), num_offsets=0), capi.MCL_ERR_INVALID_ARGUMENT, "mcl_set_ndt_map: 1 .. 32 kernel offsets"),
    "33_offsets": ({}, dict(offsets=((0, 0),) * 32, num_offsets=33), capi.MCL_ERR_INVALID_ARGUMENT, "mcl_set_ndt_map: 1 .. 32 kernel offsets"),
    "box_too_large": (dict(cells=[(0, 0), (1 << 26, 0)]), None, capi.MCL_ERR_UNSUPPORTED,
                      "mcl_set_ndt_map: the bounding box of the keys exceeds 2^26 cells (%d x 5 with its border)" % ((1 << 26) + 5)),
}


@pytest.mark.parametrize("name", sorted(NDT_REFUSALS))
def test_ndt_map_refusals_in_the_librarys_words(driver, name):
    change, params, want_status, want_message = NDT_REFUSALS[name]
    status, message, got = _ndt_map(driver, *_two_cells(**change), params=None if params is None else _ndt_params(**params))
    assert (status, message, got) == (want_status, want_message, None)


def test_ndt_two_cell_map_is_accepted_as_it_stands(driver):
    """The map the refusals start from, and the widest kernel the checks let through: reach 64."""
    assert _ndt_map(driver, *_two_cells())[0] == capi.MCL_OK
    status, _, got = _ndt_map(driver, *_two_cells(), params=_ndt_params(offsets=((0, 0), (-64, 3))))
    assert status == capi.MCL_OK and got["reach"] == 64 and (got["gw"], got["gh"]) == (2 + 256, 3 + 256)


# ---- landmark and bearing: the map --------------------------------------------------------------------------------------------------

CATEGORIES = (3, 1, 3, 2, 1, 3)
POSITIONS = np.array([(1.0, 2.0, 0.5), (-3.0, 0.25, 1.0), (4.0, -1.0, 0.0), (0.5, 0.5, 2.0), (-2.0, 3.0, -0.5), (2.5, -4.0, 1.5)])
BOUNDARIES = (-5.0, -6.0, -1.0, 7.0, 8.0, 3.0)
RANGES = {1: (0, 2), 2: (2, 1), 3: (3, 3)}
# a unit quaternion (x, y, z, w) that is no rotation about an axis of the frame: (1, 2, 3, 4) / sqrt(30), normalised once more after rounding
QUATERNION = np.array([1.0, 2.0, 3.0, 4.0]) / np.sqrt(30.0)
QUATERNION = QUATERNION / np.sqrt(np.sum(QUATERNION * QUATERNION))


def _landmark_map(driver, kind, positions, categories, boundaries=None, params=None):
    positions = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    n = len(positions)
    p = np.zeros(8)
    if params is not None:
        p[:len(params)] = params
    words = _call(driver, "lmmap", _i(kind, n, boundaries is not None, params is not None), _f(p), _f(positions), _i(*categories) if n else _i(),
                  _f(boundaries if boundaries is not None else np.zeros(6)))
    status, message, rest = _status(words)
    if status != capi.MCL_OK:
        assert len(rest) == 0
        return status, message, None
    r = rest.view(np.float64)
    got = dict(den_range=r[0], den_bearing=r[1], random_prob=r[2], Rs=r[3:12].reshape(3, 3), ts=r[12:15], lo=r[15:18], hi=r[18:21],
               landmarks=r[21:21 + 4 * n].reshape(n, 4))
    tail = rest[21 + 4 * n:]
    assert len(tail) == 1 + 3 * int(tail[0])
    got["ranges"] = {int(c): (int(f), int(k)) for c, f, k in tail[1:].reshape(-1, 3)}
    return status, message, got


def test_landmarks_are_grouped_by_category_in_map_order(driver):
    status, message, got = _landmark_map(driver, capi.MCL_SENSOR_LANDMARK, POSITIONS, CATEGORIES)
    assert (status, message) == (capi.MCL_OK, "")
    order = [1, 4, 3, 0, 2, 5]  # categories 1, 1, 2, 3, 3, 3: the input's order kept inside a category
    assert np.array_equal(got["landmarks"], np.concatenate([POSITIONS[order], np.zeros((6, 1))], 1))
    assert got["ranges"] == RANGES
    lo, hi = lref.LandmarkMap(POSITIONS, CATEGORIES).map_limits()  # without boundaries: the landmarks' bounding box
    assert np.array_equal(got["lo"], lo) and np.array_equal(got["hi"], hi)
    assert (got["den_range"], got["den_bearing"], got["random_prob"]) == (2.0, 2.0, 1e-4)  # the defaults
    assert np.all(got["Rs"] == 0.0) and np.all(got["ts"] == 0.0)
    status, _, got = _landmark_map(driver, capi.MCL_SENSOR_LANDMARK, POSITIONS, CATEGORIES, BOUNDARIES, params=(0.3, 0.7, 0.01))
    assert status == capi.MCL_OK
    assert np.array_equal(got["lo"], BOUNDARIES[:3]) and np.array_equal(got["hi"], BOUNDARIES[3:])  # with boundaries: those
    assert (got["den_range"], got["den_bearing"], got["random_prob"]) == ((2.0 * 0.3) * 0.3, (2.0 * 0.7) * 0.7, 0.01)


def test_landmark_map_refusals(driver):
    bad = list(BOUNDARIES)
    bad[0], bad[3] = bad[3], bad[0]
    assert _landmark_map(driver, capi.MCL_SENSOR_LANDMARK, POSITIONS, CATEGORIES, bad) == (
        capi.MCL_ERR_INVALID_ARGUMENT, "mcl_set_landmark_map: boundaries with min > max", None)
    assert _landmark_map(driver, capi.MCL_SENSOR_LANDMARK, np.zeros((0, 3)), ()) == (
        capi.MCL_ERR_INVALID_ARGUMENT, "mcl_set_landmark_map: an empty map needs explicit boundaries", None)
    status, _, got = _landmark_map(driver, capi.MCL_SENSOR_LANDMARK, np.zeros((0, 3)), (), BOUNDARIES)  # (with them it is a valid, empty map)
    assert status == capi.MCL_OK and got["ranges"] == {} and len(got["landmarks"]) == 0


def test_bearing_map_rotation_is_eigens_to_the_last_bit(driver):
    pose = tuple(QUATERNION) + (0.1, -0.2, 0.3)
    status, message, got = _landmark_map(driver, capi.MCL_SENSOR_BEARING, POSITIONS, CATEGORIES, params=(0.5,) + pose)
    assert (status, message) == (capi.MCL_OK, "")
    assert np.array_equal(got["Rs"], lref.rotation_matrix(QUATERNION))
    assert abs(np.linalg.det(got["Rs"]) - 1.0) < 1e-12 and not np.any(np.abs(got["Rs"]) > 0.999)  # a rotation, about no axis of the frame
    assert np.array_equal(got["ts"], pose[4:]) and got["den_bearing"] == (2.0 * 0.5) * 0.5 and got["den_range"] == 0.0
    assert got["ranges"] == RANGES
    longer = tuple(QUATERNION * (1.0 + 1e-6)) + pose[4:]
    assert _landmark_map(driver, capi.MCL_SENSOR_BEARING, POSITIONS, CATEGORIES, params=(0.5,) + longer) == (
        capi.MCL_ERR_INVALID_ARGUMENT, "mcl_set_landmark_map: sensor_pose_in_robot's quaternion is not of unit length", None)


# ---- landmark and bearing: the detection records ------------------------------------------------------------------------------------

DETECTIONS = np.array([(1.5, -2.0, 0.25), (0.0, 0.0, 0.0), (-0.75, 3.0, 1.0)])
DETECTION_CATEGORIES = (3, 9, 1)  # 9: a category the map does not have


def _records(driver, kind, xyz, categories, ranges=RANGES):
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    triples = [] if ranges is None else [(c, f, k) for c, (f, k) in sorted(ranges.items())]
    words = _call(driver, "records", _i(kind, len(xyz), -1 if ranges is None else len(triples)), _i(*triples) if triples else _i(), _f(xyz),
                  _i(*categories))
    status, message, rest = _status(words)
    if status != capi.MCL_OK:
        assert len(rest) == 0
        return status, message, None
    recs = rest.reshape(len(xyz), 10)
    return status, message, (recs[:, :7].view(np.float64), recs[:, 7:9].copy().view(np.uint32).reshape(len(xyz), 4))


def _check_records(reals, packed, order):
    d = DETECTIONS[order]
    assert np.array_equal(reals[:, :3], d)
    assert np.array_equal(reals[:, 3], lref._norm3(d[:, 0], d[:, 1], d[:, 2]))
    assert np.array_equal(reals[:, 4:7], np.stack(lref._normalized(d[:, 0], d[:, 1], d[:, 2]), 1))
    zero = order.index(1)
    assert np.array_equal(reals[zero], np.zeros(7))  # the zero vector keeps its components: no division
    want = [RANGES.get(DETECTION_CATEGORIES[i], (0xFFFFFFFF, 0)) + (i, 0) for i in order]
    assert np.array_equal(packed, np.array(want, dtype=np.uint32))
    assert tuple(packed[zero][:2]) == (0xFFFFFFFF, 0)  # the unknown category


def test_landmark_records_keep_the_callers_order(driver):
    status, message, (reals, packed) = _records(driver, capi.MCL_SENSOR_LANDMARK, DETECTIONS, DETECTION_CATEGORIES)
    assert (status, message) == (capi.MCL_OK, "")
    _check_records(reals, packed, [0, 1, 2])


def test_bearing_records_are_sorted_by_category_and_say_where_they_stood(driver):
    status, message, (reals, packed) = _records(driver, capi.MCL_SENSOR_BEARING, DETECTIONS, DETECTION_CATEGORIES)
    assert (status, message) == (capi.MCL_OK, "")
    _check_records(reals, packed, [2, 0, 1])  # categories 1, 3, 9; the third packed word is the place in the caller's order


def test_detection_records_refusals(driver):
    many = capi.MCL_LANDMARK_MAX_DETECTIONS + 1
    assert _records(driver, capi.MCL_SENSOR_LANDMARK, np.ones((many, 3)), (1,) * many) == (
        capi.MCL_ERR_INVALID_ARGUMENT, "driver: more than MCL_LANDMARK_MAX_DETECTIONS detections", None)
    status, _, (reals, _) = _records(driver, capi.MCL_SENSOR_LANDMARK, np.ones((many - 1, 3)), (1,) * (many - 1))
    assert status == capi.MCL_OK and len(reals) == capi.MCL_LANDMARK_MAX_DETECTIONS
    assert _records(driver, capi.MCL_SENSOR_BEARING, DETECTIONS, DETECTION_CATEGORIES, ranges=None) == (
        capi.MCL_ERR_NOT_READY, "driver: no landmark map set (mcl_set_landmark_map)", None)
