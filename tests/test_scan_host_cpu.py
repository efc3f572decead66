"""The one rule about which points of a scan are staged (mcl::scan_finite_points, beluga_amd/csrc/scan_host.cpp) on the CPU: a plain g++
builds the file, with one C entry point around the function, into a small shared object; the kept points, their count and the index list
are held bit for bit to a few lines of numpy.  tests/cpp/scan_host_check.cpp runs the same file as a program of its own under the
sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beluga_amd", "csrc")

SHIM = r"""
#include "scan_host.h"
extern "C" uint64_t shim_scan_finite_points(const double* points_xy, uint64_t num_points, double* kept_xy, uint32_t* slots) {
  return mcl::scan_finite_points(points_xy, num_points, kept_xy, slots);
}
"""

SIZES = (0, 1, 2, 7, 64)
SENTINEL_BITS = 0x7FF8DEADBEEF0001  # a NaN no input holds: what the function leaves alone keeps these bits
SENTINEL_SLOT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("scan_host")
    shim, out = d / "shim.cpp", d / "libscan_host.so"
    shim.write_text(SHIM)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(CSRC, "scan_host.cpp"), str(shim), "-o", str(out)])
    so = C.CDLL(str(out))
    so.shim_scan_finite_points.restype = C.c_uint64
    so.shim_scan_finite_points.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    return so


def clean_scan(n):
    rng = np.random.default_rng(1000 + n)
    p = rng.uniform(-30.0, 30.0, size=(n, 2))
    if n:
        p[0] = (-0.0, 5e-324)  # a signed zero and a denormal: finite, and their bits must come through
    return p


def scans(n):
    """name -> scan of n points, for every input the rule has to get right at this size."""
    out = {"nothing_to_take_out": clean_scan(n)}
    if n == 0:
        return out
    for name, column, value, rows in (("nan_in_x_only", 0, np.nan, [n // 2]),
                                      ("infinity_in_y_only", 1, np.inf, [n // 2]),
                                      ("negative_infinity_in_y_only", 1, -np.inf, [n // 2]),
                                      ("first_point", 0, np.nan, [0]),
                                      ("last_point", 1, np.inf, [n - 1]),
                                      ("first_and_last_point", 0, -np.inf, [0, n - 1]),
                                      ("every_point", 1, np.nan, list(range(n))),
                                      ("every_other_point", 0, np.inf, list(range(0, n, 2)))):
        p = clean_scan(n)
        p[rows, column] = value
        out[name] = p
    p = clean_scan(n)
    p[n // 2] = (1e308, 1e308)  # finite; |x| + |y| overflows; the point stays
    p[n - 1] = (-1e308, 1e308)
    out["sum_overflows"] = p
    if n >= 2:
        p = p.copy()
        p[0, 0] = np.nan
        out["sum_overflows_beside_a_nan"] = p
    return out


def run(lib, points, with_slots):
    n = len(points)
    src = np.ascontiguousarray(points, dtype=np.float64).reshape(-1)
    before = src.copy()
    kept = np.full(2 * n + 2, SENTINEL_BITS, dtype=np.uint64)  # (one point of room behind: nothing is written there)
    slots = np.full(n + 1, SENTINEL_SLOT, dtype=np.uint32)
    count = lib.shim_scan_finite_points(src.ctypes.data if n else None, n, kept.ctypes.data, slots.ctypes.data if with_slots else None)
    assert np.array_equal(src.view(np.uint64), before.view(np.uint64))  # the scan is read only
    return count, kept, slots


CASES = [(n, name) for n in SIZES for name in scans(n)]


@pytest.mark.parametrize("n,name", CASES, ids=[f"{n}-{name}" for n, name in CASES])
def test_kept_points_count_and_index_list(lib, n, name):
    points = scans(n)[name]
    mask = np.isfinite(points[:, 0]) & np.isfinite(points[:, 1]) if n else np.zeros(0, dtype=bool)
    want = np.ascontiguousarray(points[mask]).reshape(-1).view(np.uint64)
    want_slots = np.nonzero(mask)[0].astype(np.uint32)
    if name == "nothing_to_take_out" or name == "sum_overflows":
        assert mask.all()
    if name == "every_point":
        assert not mask.any()
    for with_slots in (True, False):
        count, kept, slots = run(lib, points, with_slots)
        assert count == int(mask.sum())
        assert np.array_equal(kept[:2 * count], want)  # bit for bit, in the caller's order
        assert (kept[2 * count:] == SENTINEL_BITS).all()
        if with_slots:
            assert np.array_equal(slots[:count], want_slots)
            assert (slots[count:] == SENTINEL_SLOT).all()
        else:
            assert (slots == SENTINEL_SLOT).all()


def test_the_stand_alone_check_passes_under_the_sanitizers(tmp_path):
    """tests/cpp/scan_host_check.cpp with scan_host.cpp, as a program of its own under the address and undefined-behaviour sanitizers:
    nothing of it is loaded into this process."""
    exe = tmp_path / "scan_host_check"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "scan_host_check.cpp"),
                           os.path.join(CSRC, "scan_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "scan_host_check OK", out.stdout + out.stderr
