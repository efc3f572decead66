"""The host rule of mcl_cast_rays* (beluga_amd/csrc/raycast_host.cpp) on the CPU: a plain g++ builds the file, with a few C entry
points around its functions, into a small shared object; the checks are held at their edges and the chunk plan to
tests/raycast_reference.py.  tests/cpp/raycast_host_check.cpp runs the same file as a program of its own under the sanitizers."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import raycast_reference as rc
from beluga_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beluga_amd", "csrc")

SHIM = r"""
#include "raycast_host.h"
extern "C" {
int shim_check_range(double max_range, double resolution) { return mcl::cast_check_range(max_range, resolution) ? 1 : 0; }
int shim_check_call(const double* poses, int look, int have_poses, uint64_t n, const double* bearings, uint64_t B, double max_range,
                    double resolution, int have_ranges) {
  const char* what = nullptr;
  return mcl::cast_check_call(poses, look != 0, have_poses != 0, n, bearings, B, max_range, resolution, have_ranges != 0, &what);
}
uint64_t shim_plan(uint64_t n, uint64_t B, uint64_t chunk, uint64_t* head, uint64_t* rows, uint64_t capacity) {
  const mcl::CastPlan plan = mcl::cast_plan(n, B, chunk);
  head[0] = plan.rays, head[1] = plan.chunk_rays, head[2] = plan.chunks, head[3] = plan.chunk_poses;
  for (uint64_t c = 0; c < plan.chunks && c < capacity; ++c) {
    const mcl::CastChunk k = mcl::cast_chunk_at(plan, B, c);
    const uint64_t row[6] = {k.first_ray, k.rays, k.first_pose, k.first_bearing, k.poses, k.blocks};
    for (int j = 0; j < 6; ++j) rows[6 * c + j] = row[j];
  }
  return plan.chunks;
}
}
"""

BOUND_CELLS = 2.0 ** 27 - 2.0
RES = 0.0625  # (an exact reciprocal: max_range / resolution is exact)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("raycast_host")
    shim, out = d / "shim.cpp", d / "libraycast_host.so"
    shim.write_text(SHIM)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(CSRC, "raycast_host.cpp"), str(shim), "-o", str(out)])
    so = C.CDLL(str(out))
    so.shim_check_range.restype = C.c_int
    so.shim_check_range.argtypes = [C.c_double, C.c_double]
    so.shim_check_call.restype = C.c_int32
    so.shim_check_call.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_int]
    so.shim_plan.restype = C.c_uint64
    so.shim_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, capi.c_u64_p, capi.c_u64_p, C.c_uint64]
    return so


def check_call(lib, poses, bearings, max_range=2.0, look=True, have_poses=True, have_ranges=True, n=None, B=None):
    p = None if poses is None else np.ascontiguousarray(poses, dtype=np.float64)
    b = None if bearings is None else np.ascontiguousarray(bearings, dtype=np.float64)
    return lib.shim_check_call(None if p is None else p.ctypes.data, int(look), int(have_poses and p is not None),
                               (len(p) if n is None else n), None if b is None else b.ctypes.data, (len(b) if B is None else B), max_range, RES,
                               int(have_ranges))


def plan(lib, n, B, chunk, capacity=4096):
    head = (C.c_uint64 * 4)()
    rows = (C.c_uint64 * (6 * capacity))()
    chunks = lib.shim_plan(n, B, chunk, head, rows, capacity)
    return list(head), [tuple(rows[6 * c: 6 * c + 6]) for c in range(min(chunks, capacity))]


def test_max_range_one_step_either_side_of_the_reach_bound(lib):
    bound = BOUND_CELLS * RES
    assert lib.shim_check_range(math.nextafter(bound, 0.0), RES) == 0
    assert lib.shim_check_range((BOUND_CELLS - 1.0) * RES, RES) == 0  # one cell below
    assert lib.shim_check_range(bound, RES) == 1
    assert lib.shim_check_range(math.nextafter(bound, math.inf), RES) == 1
    assert rc.MAX_REACH_CELLS == BOUND_CELLS
    for bad in (0.0, -0.0, -1.0, math.inf, -math.inf, math.nan):
        assert lib.shim_check_range(bad, RES) == 1, bad
    assert lib.shim_check_range(5e-324, RES) == 0


POSES = [[1.0, 0.0, 0.5, 0.5], [0.0, 1.0, -3.0, 2.0]]
BEARINGS = [[1.0, 0.0], [0.6, 0.8], [0.0, -1.0]]


def test_values_that_are_not_finite_and_null_arguments(lib):
    assert check_call(lib, POSES, BEARINGS) == capi.MCL_OK
    for bad in (math.inf, -math.inf, math.nan):
        for k in range(8):
            p = np.array(POSES)
            p.flat[k] = bad
            assert check_call(lib, p, BEARINGS) == capi.MCL_ERR_INVALID_ARGUMENT
            assert check_call(lib, p, BEARINGS, look=False) == capi.MCL_OK  # the device form cannot look at the poses
        for k in range(6):
            b = np.array(BEARINGS)
            b.flat[k] = bad
            assert check_call(lib, POSES, b) == capi.MCL_ERR_INVALID_ARGUMENT
            assert check_call(lib, POSES, b, look=False) == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.shim_check_call(None, 1, 0, 2, np.array(BEARINGS).ctypes.data, 3, 2.0, RES, 1) == capi.MCL_ERR_INVALID_ARGUMENT
    assert check_call(lib, POSES, None, B=3) == capi.MCL_ERR_INVALID_ARGUMENT
    assert check_call(lib, POSES, BEARINGS, have_ranges=False) == capi.MCL_ERR_INVALID_ARGUMENT
    assert check_call(lib, POSES, BEARINGS, max_range=BOUND_CELLS * RES) == capi.MCL_ERR_INVALID_ARGUMENT


def test_zero_counts_are_ok_and_look_at_nothing(lib):
    for n, B in ((0, 0), (0, 3), (2, 0)):
        assert lib.shim_check_call(None, 1, 0, n, None, B, 2.0, RES, 0) == capi.MCL_OK
        assert lib.shim_check_call(None, 1, 0, n, None, B, math.nan, RES, 0) == capi.MCL_ERR_INVALID_ARGUMENT  # max_range all the same
        head, rows = plan(lib, n, B, 64)
        assert head[0] == 0 and head[2] == 0 and rows == []


def test_counts_no_memory_holds_are_refused_before_anything_is_read(lib):
    b = np.array(BEARINGS).ctypes.data
    for n, B in ((2 ** 40 + 1, 1), (1, 2 ** 36 + 1), (2 ** 40, 2 ** 30), (2 ** 64 - 1, 2 ** 64 - 1)):
        assert lib.shim_check_call(None, 0, 1, n, b, B, 2.0, RES, 1) == capi.MCL_ERR_OUT_OF_MEMORY


@pytest.mark.parametrize("n,B", [(1, 1), (3, 129), (65, 7), (1, 4097), (5, 1), (7, 64), (2000, 180), (1000, 360)])
def test_the_chunk_plan_around_cast_chunk(lib, n, B):
    rays = n * B
    for chunk in sorted({0, 1, 63, 64, 65, 100, 255, 256, 257, 4096, 4097, rays - 1, rays, rays + 1, B - 1, B, B + 1, 2 * B + 1, 1 << 22}):
        if chunk < 0 or rays // max(chunk, 64) > 4000:
            continue
        head, rows = plan(lib, n, B, chunk)
        want = rc.chunk_plan(n, B, chunk)
        assert head[0] == rays and head[1] == min(max(chunk, 64), 1 << 38) and head[2] == len(want)
        assert rows == want, (n, B, chunk)
        assert max(r[4] for r in rows) <= head[3] <= n  # the pose area holds what any chunk touches


def test_the_chunk_plan_around_the_grid_limit(lib):
    """A launch holds 2^30 workgroups of 256 rays (below a grid dimension's 2^31 - 1): the device form's chunk."""
    launch = (1 << 30) * 256
    B = 1 << 19
    for extra in (0, 1):
        n = launch // B + extra
        head, rows = plan(lib, n, B, launch)
        assert head[2] == 1 + extra and rows[0] == (0, launch, 0, 0, launch // B, 1 << 30)
        if extra:
            assert rows[1] == (launch, B, n - 1, 0, 1, B // 256)
    head, rows = plan(lib, launch + 1, 1, 2 ** 64 - 1)  # a chunk above a launch's size is a launch's size
    assert head[1] == launch and rows == [(0, launch, 0, 0, launch, 1 << 30), (launch, 1, launch, 0, 1, 1)]
    head, rows = plan(lib, 3, launch - 1, launch)  # a chunk that is no multiple of the table: the later ones start inside a pose
    assert rows[1] == (launch, launch, 1, 1, 2, 1 << 30) and rows[2][1] == 3 * (launch - 1) - 2 * launch and rows[2][4] == 1


def test_the_option_table_takes_cast_chunk(tmp_path):
    src = tmp_path / "driver.cpp"
    src.write_text(r"""
#include <cstdio>
#include <cstdlib>
#include "options_host.h"
#include "raycast_host.h"
int main(int argc, char** argv) {
  mcl::Tuning t;
  std::printf("%d", t.cast_chunk);
  if (t.cast_chunk != mcl::kCastChunkDefault) return 1;
  for (int i = 1; i < argc; ++i) {
    const bool ok = mcl::set_tuning(t, "cast_chunk", std::strtoll(argv[i], nullptr, 10));
    std::printf(" %d:%d", ok ? 1 : 0, t.cast_chunk);
  }
  return 0;
}
""")
    exe = tmp_path / "driver"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), os.path.join(CSRC, "options_host.cpp"),
                           "-o", str(exe)])
    out = subprocess.check_output([str(exe), "0", "63", "64", "4096", str(2 ** 28), str(2 ** 28 + 1), str(2 ** 40)], text=True)
    assert out == "4194304 1:64 1:64 1:64 1:4096 1:268435456 1:268435456 1:268435456"


def test_the_stand_alone_check_passes_under_the_sanitizers(tmp_path):
    """tests/cpp/raycast_host_check.cpp with raycast_host.cpp, as a program of its own under the address and undefined-behaviour
    sanitizers: nothing of it is loaded into this process."""
    exe = tmp_path / "raycast_host_check"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "raycast_host_check.cpp"),
                           os.path.join(CSRC, "raycast_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "raycast_host_check OK", out.stdout + out.stderr
