"""The pivot of the estimate sums as a fact about the live set (beluga_amd/csrc/set_facts.h) on the CPU: a plain g++ compiles the header
with a short driver - with the address and undefined-behaviour sanitizers, as a stand-alone program - that plays events and prints the
pivot after each.  The assertions are the pivot's column of the header's event table."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
// driver event[:x,y] ...   One line per event: <known> <x> <y> (hex floats)
#include <cstdio>
#include <cstdlib>
#include <string>

#include "cycle_host.h"
#include "set_facts.h"

int main(int argc, char** argv) {
  mcl::SetFacts f;
  for (int k = 1; k < argc; ++k) {
    std::string name(argv[k]);
    double a[4] = {0, 0, 0, 0};
    if (const size_t colon = name.find(':'); colon != std::string::npos) {
      const char* p = argv[k] + colon + 1;
      for (int j = 0; j < 4 && *p; ++j) {
        char* end = nullptr;
        a[j] = std::strtod(p, &end);
        p = *end ? end + 1 : end;
      }
      name.resize(colon);
    }
    if (name == "set_changes") f.set_changes();
    else if (name == "set_replaced") f.set_replaced(a[0] != 0, a[1] != 0);
    else if (name == "set_resized") f.set_resized(a[0] != 0);
    else if (name == "pivot_given") f.pivot_given(a[0], a[1]);
    else if (name == "estimate_reported") f.estimate_reported(a[0], a[1], a[2], a[3]);  // (c, s, x, y)
    else if (name == "pivot_carried") f.pivot_carried(a[0], a[1], a[2], a[3]);  // (dc, ds, tx, ty)
    else if (name == "needs_repivot") { double t[12] = {a[0], 0, 0, 0, a[1], 0, a[2], 0, a[3], 0, 0, 0}; std::printf("%d ", mcl::estimate_needs_repivot(t) ? 1 : 0); }
    else if (name == "resampled_set_committed") f.resampled_set_committed();
    else if (name == "commit_rolled_back") f.commit_rolled_back();
    else if (name == "weights_touched") f.weights_touched();
    else return 2;
    std::printf("%d %a %a\n", f.pivot_known() ? 1 : 0, f.pivot()[0], f.pivot()[1]);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("set_facts_pivot")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "beluga_amd", "csrc"), "-I", os.path.join(ROOT, "include"), str(src),
                           os.path.join(ROOT, "beluga_amd", "csrc", "cycle_host.cpp"), "-o", str(exe)])
    return str(exe)


def last(driver, *events):
    out = subprocess.check_output([driver] + list(events), text=True).splitlines()
    assert len(out) == len(events)
    known, x, y = out[-1].split()
    return int(known), float.fromhex(x), float.fromhex(y)


def test_a_fresh_context_has_no_pivot_and_sums_about_the_origin(driver):
    assert last(driver, "set_changes") == (0, 0.0, 0.0)


def test_a_given_pivot_stands_until_the_set_is_replaced(driver):
    assert last(driver, "pivot_given:5e5,4e6") == (1, 5e5, 4e6)
    for keeps in ("set_changes", "set_resized:0", "set_resized:1", "resampled_set_committed", "commit_rolled_back", "weights_touched"):
        assert last(driver, "pivot_given:5e5,4e6", keeps) == (1, 5e5, 4e6), keeps
    for unit in (0, 1):
        assert last(driver, "pivot_given:5e5,4e6", f"set_replaced:{unit}") == (0, 0.0, 0.0)


def test_an_estimate_moves_the_pivot_and_one_that_is_not_finite_does_not(driver):
    assert last(driver, "pivot_given:1,2", "estimate_reported:1,0,3.5,-4.25") == (1, 3.5, -4.25)
    assert last(driver, "estimate_reported:1,0,3.5,-4.25") == (1, 3.5, -4.25)
    for bad in ("nan,1", "1,nan", "inf,0", "0,-inf"):
        assert last(driver, "pivot_given:1,2", f"estimate_reported:1,0,{bad}") == (1, 1.0, 2.0), bad
        assert last(driver, f"pivot_given:{bad}") == (0, 0.0, 0.0), bad


def test_the_estimate_of_the_old_set_does_not_serve_the_new_one(driver):
    assert last(driver, "estimate_reported:1,0,-4e6,5e5", "set_replaced:0") == (0, 0.0, 0.0)
    assert last(driver, "estimate_reported:1,0,-4e6,5e5", "set_replaced:0", "pivot_given:5e5,4e6") == (1, 5e5, 4e6)


def test_a_shard_keeps_the_pivot_every_rank_agrees_on(driver):
    for unit in (0, 1):
        assert last(driver, "estimate_reported:1,0,-4e6,5e5", f"set_replaced:{unit},1") == (1, -4e6, 5e5)
    assert last(driver, "set_replaced:1,1") == (0, 0.0, 0.0)  # (nothing to keep on a fresh context)
    # ... and its heading: the next control action still carries it
    assert last(driver, "estimate_reported:0,1,10,20", "set_replaced:1,1", "pivot_carried:1,0,0.5,0") == (1, 10.0, 20.5)


def test_the_control_action_carries_an_estimated_pivot_and_leaves_a_given_one(driver):
    # heading +90 degrees: half a metre ahead is half a metre up; the action's rotation turns the heading for the next one
    assert last(driver, "estimate_reported:0,1,10,20", "pivot_carried:0,1,0.5,0.25") == (1, 9.75, 20.5)
    assert last(driver, "estimate_reported:0,1,10,20", "pivot_carried:0,1,0.5,0", "pivot_carried:1,0,1,0") == (1, 9.0, 20.5)
    assert last(driver, "pivot_given:10,20", "pivot_carried:1,0,0.5,0") == (1, 10.0, 20.0)
    assert last(driver, "pivot_carried:1,0,0.5,0") == (0, 0.0, 0.0)
    assert last(driver, "estimate_reported:nan,0,10,20", "pivot_carried:1,0,0.5,0") == (1, 10.0, 20.0)
    assert last(driver, "estimate_reported:0,1,10,20", "pivot_carried:1,0,nan,0") == (1, 10.0, 20.0)


def needs(driver, w, swdx, swdxdx, swdydy):
    out = subprocess.check_output([driver, f"needs_repivot:{w},{swdx},{swdxdx},{swdydy}"], text=True).split()
    return int(out[0])


def test_the_second_pass_is_taken_where_the_mean_offset_exceeds_three_variances(driver):
    """estimate_needs_repivot (cycle_host.h): |m|^2 > 3 T, T = M - |m|^2, written as 4 |m|^2 > 3 M."""
    # W = 2, m = 1, M = 1 + T
    assert needs(driver, 2, 2, 2 * (1 + 0.34), 0) == 0      # T = 0.34: |m|^2 = 1 < 1.02
    assert needs(driver, 2, 2, 2 * (1 + 0.33), 0) == 1      # T = 0.33: 1 > 0.99
    assert needs(driver, 2, 2, 2 * 0.5, 2 * (0.5 + 0.33)) == 1  # (the trace: both axes count)
    assert needs(driver, 1, 0, 0, 0) == 0                   # one particle at the pivot
    assert needs(driver, 1, 4e6, 1.6e13, 0) == 1            # all the mass 4e6 m from the pivot
    assert needs(driver, 0, 1, 1, 1) == 0 and needs(driver, 1, "nan", 1, 1) == 0 and needs(driver, 1, 1, "inf", 1) == 0
