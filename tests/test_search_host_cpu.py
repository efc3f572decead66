"""The global pose search's host rule (beluga_amd/csrc/search_host.cpp) on the CPU: a plain g++ builds the file into a small shared
object, and mcl_search_suppress, the parameter checks and the defaults are held to tests/search_reference.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import search_reference as ref
from beluga_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("search_host") / "libsearch_host.so"
    csrc = os.path.join(ROOT, "beluga_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I", csrc, "-I", os.path.join(ROOT, "include"),
                           os.path.join(csrc, "search_host.cpp"), "-o", str(out)])
    so = C.CDLL(str(out))
    so.mcl_default_search_params.restype = None
    so.mcl_default_search_params.argtypes = [C.POINTER(capi.SearchParams)]
    so.mcl_search_suppress.restype = C.c_int32
    so.mcl_search_suppress.argtypes = capi._SIGNATURES["mcl_search_suppress"][1]
    return so


def make_pool(entries, headings):
    pool = (capi.SearchHit * max(len(entries), 1))()
    for hit, (cell, h) in zip(pool, entries):
        hit.cell, hit.heading, hit.id = cell, h, cell * headings + h
    return pool


def suppress(lib, entries, width, params):
    pool = make_pool(entries, params.headings)
    kept = (C.c_uint32 * 4100)(*([0xFFFFFFFF] * 4100))
    n = C.c_uint64(12345)
    status = lib.mcl_search_suppress(pool, len(entries), width, C.byref(params), kept, C.byref(n))
    return status, list(kept[: n.value]) if status == 0 else None, (list(kept), n.value)


def check(lib, entries, width, params):
    status, kept, _ = suppress(lib, entries, width, params)
    assert status == capi.MCL_OK
    want = ref.suppress([e[0] for e in entries], [e[1] for e in entries], width, params.headings, params.separation_cells,
                        params.separation_headings, params.max_results)
    assert kept == want
    return kept


P = capi.SearchParams
W = 50


def cell(x, y):
    return y * W + x


def test_defaults(lib):
    p = P()
    lib.mcl_default_search_params(C.byref(p))
    assert [getattr(p, n) for n, _ in P._fields_] == [2, 72, 1024, 16, 10, 6]
    lib.mcl_default_search_params(None)


def test_zero_separations_drop_nothing(lib):
    entries = [(cell(5, 5), 0), (cell(5, 5), 1), (cell(6, 5), 0), (cell(5, 5), 7), (cell(5, 6), 0)]
    assert check(lib, entries, W, P(1, 8, 5, 5, 0, 0)) == [0, 1, 2, 3, 4]


def test_distance_exactly_at_the_bound_and_one_more(lib):
    # separation_cells 5: (3, 4) and (0, 5) lie at squared distance 25 (dropped), (3, 5) at 34 and (5, -1) at 26 (kept)
    entries = [(cell(10, 10), 2), (cell(13, 14), 2), (cell(13, 15), 2), (cell(15, 9), 2), (cell(10, 15), 2)]
    assert check(lib, entries, W, P(1, 8, 8, 8, 5, 0)) == [0, 2, 3]
    # near in cells but not in heading: kept (the rule is AND)
    entries = [(cell(10, 10), 0), (cell(11, 10), 3), (cell(11, 10), 2), (cell(40, 40), 0)]
    assert check(lib, entries, W, P(1, 8, 8, 8, 5, 2)) == [0, 1, 3]


def test_heading_wrap(lib):
    entries = [(cell(10, 10), 71), (cell(10, 10), 0), (cell(10, 10), 2), (cell(10, 10), 69), (cell(10, 10), 3), (cell(10, 10), 36)]
    assert check(lib, entries, W, P(1, 72, 8, 8, 0, 1)) == [0, 2, 3, 5]
    assert check(lib, entries, W, P(1, 72, 8, 8, 3, 3)) == [0, 4, 5]


def test_one_and_two_headings(lib):
    assert check(lib, [(cell(1, 1), 0), (cell(2, 1), 0), (cell(9, 9), 0)], W, P(1, 1, 4, 4, 1, 0)) == [0, 2]
    entries = [(cell(1, 1), 0), (cell(1, 1), 1), (cell(2, 1), 1)]
    assert check(lib, entries, W, P(1, 2, 4, 4, 1, 0)) == [0, 1]
    assert check(lib, entries, W, P(1, 2, 4, 4, 1, 1)) == [0]  # min(1, 2 - 1) = 1


def test_max_results_and_pool_sizes(lib):
    rng = np.random.default_rng(4)
    entries = [(cell(int(x), int(y)), int(h)) for x, y, h in zip(rng.integers(0, W, 64), rng.integers(0, 40, 64), rng.integers(0, 16, 64))]
    assert check(lib, entries, W, P(1, 16, 64, 1, 10, 3)) == [0]
    assert len(check(lib, entries, W, P(1, 16, 64, 64, 0, 0))) == 64  # max_results == pool
    check(lib, entries, W, P(1, 16, 64, 64, 6, 2))
    check(lib, entries, W, P(1, 16, 64, 7, 6, 2))
    assert check(lib, entries[:1], W, P(1, 16, 1, 1, 10, 3)) == [0]  # a pool of one
    assert check(lib, [], W, P(1, 16, 4, 4, 10, 3)) == []


def test_a_pool_whose_entries_all_tie_is_decided_by_position(lib):
    # equal scores: the pool order is the id order, and the rule reads cells and headings alone
    entries = [(cell(x, 3), 0) for x in range(0, 40)]
    assert check(lib, entries, W, P(1, 4, 64, 64, 4, 0)) == [0, 5, 10, 15, 20, 25, 30, 35]


def test_refusals_write_nothing(lib):
    entries = [(cell(1, 1), 0), (cell(9, 9), 1)]
    bad = [P(0, 8, 16, 4, 0, 0), P(1, 0, 16, 4, 0, 0), P(1, 4097, 16, 4, 0, 0), P(1, 8, 0, 1, 0, 0), P(1, 8, 4097, 4, 0, 0), P(1, 8, 16, 0, 0, 0),
           P(1, 8, 16, 17, 0, 0), P(1, 1, 16, 4, 0, 0)]  # (the last: a heading >= headings)
    for params in bad:
        status, _, (kept, n) = suppress(lib, entries, W, params)
        assert status == capi.MCL_ERR_INVALID_ARGUMENT and n == 12345 and all(k == 0xFFFFFFFF for k in kept), list(bytes(params))
    good = P(1, 8, 16, 4, 0, 0)
    pool = make_pool(entries, 8)
    kept_buf = (C.c_uint32 * 4)()
    count = C.c_uint64(12345)
    assert lib.mcl_search_suppress(pool, 2, 0, C.byref(good), kept_buf, C.byref(count)) == capi.MCL_ERR_INVALID_ARGUMENT  # grid_width 0
    assert lib.mcl_search_suppress(None, 2, W, C.byref(good), kept_buf, C.byref(count)) == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.mcl_search_suppress(pool, 2, W, C.byref(good), None, C.byref(count)) == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.mcl_search_suppress(pool, 2, W, C.byref(good), kept_buf, None) == capi.MCL_ERR_INVALID_ARGUMENT
    assert count.value == 12345
    assert lib.mcl_search_suppress(pool, 2, W, None, kept_buf, C.byref(count)) == capi.MCL_OK and count.value == 2  # NULL: the defaults


def test_the_option_table_takes_search_chunk(tmp_path):
    src = tmp_path / "driver.cpp"
    src.write_text(r"""
#include <cstdio>
#include <cstdlib>
#include "options_host.h"
int main(int argc, char** argv) {
  mcl::Tuning t;
  std::printf("%d", t.search_chunk);
  for (int i = 1; i < argc; ++i) {
    const bool ok = mcl::set_tuning(t, "search_chunk", std::strtoll(argv[i], nullptr, 10));
    std::printf(" %d:%d", ok ? 1 : 0, t.search_chunk);
  }
  return 0;
}
""")
    csrc = os.path.join(ROOT, "beluga_amd", "csrc")
    exe = tmp_path / "driver"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", csrc, str(src), os.path.join(csrc, "options_host.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe), "0", "63", "64", "4096", str(2 ** 22), str(2 ** 22 + 1), str(2 ** 40)], text=True)
    assert out == "1048576 1:64 1:64 1:64 1:4096 1:4194304 1:4194304 1:4194304"


def test_the_stand_alone_check_passes_under_the_sanitizers(tmp_path):
    """tests/cpp/search_host_check.cpp with search_host.cpp, as a program of its own under the address and undefined-behaviour
    sanitizers: nothing of it is loaded into this process."""
    exe = tmp_path / "search_host_check"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "beluga_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "search_host_check.cpp"), os.path.join(ROOT, "beluga_amd", "csrc", "search_host.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "search_host_check OK", out.stdout + out.stderr
