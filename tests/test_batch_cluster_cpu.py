"""Which fused members of a batch share the cluster-based estimate's two launches, and how many launches a cycle counts
(beluga_amd/csrc/batch_host.cpp), on the CPU in the manner of test_batch_cpu.py: a plain g++ compiles the file with a short driver, once
more under the address and undefined-behaviour sanitizers as a program of its own.  And the ABI surface: the switch is the members'
option batch_cluster_fused of mcl_set_option and the counters are mcl_batch_get_counter's; their error codes on null handles."""
import ctypes as C
import os
import subprocess

import pytest

from beluga_amd import build as mcl_build
from beluga_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
// driver <members>  then per member: status kind cluster_fused n linear angular percentile
//   -> a line with the picked indices (or "-"), then a line "cells_launch sums_launch_if_all_have_winners none_has_a_winner":
//      batch_cluster_launches(picked, picked), batch_cluster_launches(picked, 0)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "batch_host.h"

using namespace mcl;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  char** arg = argv + 1;
  const uint32_t members = static_cast<uint32_t>(std::strtoul(*arg++, nullptr, 0));
  if (argc != 2 + 7 * static_cast<int>(members)) return 2;
  std::vector<BatchClusterFacts> m(members);
  for (auto& f : m) {
    f.status = static_cast<int>(std::strtol(*arg++, nullptr, 0));
    f.estimate_kind = static_cast<int>(std::strtol(*arg++, nullptr, 0));
    f.cluster_fused = std::strtol(*arg++, nullptr, 0) != 0;
    f.n = std::strtoull(*arg++, nullptr, 0);
    f.linear_hash_resolution = std::strtod(*arg++, nullptr);
    f.angular_hash_resolution = std::strtod(*arg++, nullptr);
    f.weight_cap_percentile = std::strtod(*arg++, nullptr);
  }
  std::vector<uint32_t> picked(members + 1);
  const uint32_t count = batch_cluster_select(m.data(), members, picked.data());
  if (count == 0) std::printf("-");
  for (uint32_t k = 0; k < count; ++k) std::printf("%u ", picked[k]);
  std::printf("\n%u %u\n", batch_cluster_launches(count, count), batch_cluster_launches(count, 0));
  return 0;
}
"""


def _compile(tmp, name, extra):
    src = tmp / "driver.cpp"
    src.write_text(DRIVER)
    exe = tmp / name
    csrc = os.path.join(ROOT, "beluga_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror"] + extra +
                          ["-I", csrc, "-I", os.path.join(ROOT, "include"), str(src), os.path.join(csrc, "batch_host.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("batch_cluster_host"), "driver", [])


MCL_OK, MCL_ERR_HIP = 0, capi.MCL_ERR_HIP
GOOD = dict(status=MCL_OK, kind=1, fused=1, n=2000, linear=0.2, angular=0.524, percentile=0.9)


def args_of(members):
    out = [str(len(members))]
    for m in members:
        out += [str(m["status"]), str(m["kind"]), str(m["fused"]), str(m["n"]), repr(m["linear"]), repr(m["angular"]), repr(m["percentile"])]
    return out


def run(exe, members):
    lines = subprocess.check_output([exe] + args_of(members), text=True).splitlines()
    picked = [] if lines[0].strip() == "-" else [int(w) for w in lines[0].split()]
    return picked, [int(w) for w in lines[1].split()]


# the description, whether the member takes the shared launches
MEMBERS = [
    (dict(), True),
    (dict(kind=0), False),
    (dict(fused=0), False),
    (dict(n=0), False), (dict(n=1), True), (dict(n=4096), True), (dict(n=4097), False),
    (dict(status=MCL_ERR_HIP), False), (dict(status=capi.MCL_ERR_NOT_READY), False),
    (dict(linear=0.0), False), (dict(linear=-0.2), False), (dict(angular=0.0), False), (dict(linear=float("nan")), False),
    (dict(percentile=1.0), False), (dict(percentile=-0.1), False), (dict(percentile=0.0), True), (dict(percentile=float("nan")), False),
]


@pytest.mark.parametrize("change,takes", MEMBERS)
def test_every_condition_flips_alone(driver, change, takes):
    picked, launches = run(driver, [dict(GOOD, **change)])
    assert picked == ([0] if takes else [])
    assert launches == ([2, 1] if takes else [0, 0])


def test_selection_keeps_the_order_and_the_switch_empties_it(driver):
    members = [dict(GOOD, **change) for change, _ in MEMBERS]
    want = [i for i, (_, takes) in enumerate(MEMBERS) if takes]
    picked, launches = run(driver, members)
    assert picked == want and launches == [2, 1]
    picked, launches = run(driver, [dict(m, fused=0) for m in members])
    assert picked == [] and launches == [0, 0]
    assert run(driver, []) == ([], [0, 0])
    only_others = [dict(GOOD, kind=0), dict(GOOD, n=5000), dict(GOOD, status=MCL_ERR_HIP)]
    assert run(driver, only_others) == ([], [0, 0])


def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = _compile(tmp_path, "driver_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    members = [dict(GOOD, **change) for change, _ in MEMBERS]
    for args in (args_of(members), args_of([dict(m, fused=0) for m in members]), args_of([]), args_of([GOOD] * 64)):
        done = subprocess.run([exe] + args, capture_output=True, text=True)
        assert done.returncode == 0 and "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr, (args, done.stderr)


# ---- header and bindings ----------------------------------------------------------------------------------------------------------------------
def test_the_switch_is_a_member_option_and_null_handles_are_refused():
    text = open(os.path.join(ROOT, "include", "beluga_mcl.h")).read()
    for word in ("batch_cluster_fused", "cluster_launches", "members_cluster_fused"):
        assert word in text
    mcl_build.build()
    lib = capi.load()
    # null handles: refused before anything is touched
    assert lib.mcl_set_option(None, b"batch_cluster_fused", 0) == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.mcl_batch_get_counter(None, None, None) == capi.MCL_ERR_INVALID_ARGUMENT
    value = C.c_uint64(7)
    for name in (b"cluster_launches", b"members_cluster_fused"):
        assert lib.mcl_batch_get_counter(None, name, C.byref(value)) == capi.MCL_ERR_INVALID_ARGUMENT and value.value == 7
