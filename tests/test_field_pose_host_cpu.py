"""The field-frame poses of the live set on the host (option lf_pose_ahead): the fact "field poses current for map generation G"
(beluga_amd/csrc/set_facts.h) under every transition that sets or voids it, and the two decisions taken from it
(beluga_amd/csrc/cycle_host.cpp: does a propagation store them, does a likelihood-field launch load them and run k_field_pose first).
A plain g++ compiles the sources with a short driver that plays a sequence of events and prints, after each one, what the fact says
for generations 0 .. 2 and what an LF launch would do under generation 1."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
// driver [option=<0|1>] [buffer=<0|1>] event[:a] ...   One line per event: <current for G = 0> <G = 1> <G = 2> <load> <rebuild first>
// (the last two: field_pose_plan under map generation 1).  writes:<have_map> prints propagation_writes_field_poses instead.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "cycle_host.h"
#include "set_facts.h"

using namespace mcl;

int main(int argc, char** argv) {
  SetFacts f;
  Tuning t;
  bool buffer = true;
  for (int k = 1; k < argc; ++k) {
    std::string name(argv[k]);
    unsigned long long a = 0;
    if (const size_t eq = name.find('='); eq != std::string::npos) {
      const int v = std::atoi(argv[k] + eq + 1);
      name.resize(eq);
      if (name == "option") {
        if (!(t.lf_pose_ahead == 1)) return 3;  // the default
        t.lf_pose_ahead = v;
      } else if (name == "buffer") buffer = v != 0;
      else return 2;
      continue;
    }
    if (const size_t colon = name.find(':'); colon != std::string::npos) {
      a = std::strtoull(argv[k] + colon + 1, nullptr, 10);
      name.resize(colon);
    }
    if (name == "writes") {
      std::printf("%d\n", propagation_writes_field_poses(t, buffer, a != 0) ? 1 : 0);
      continue;
    }
    if (name == "field_poses_written") f.field_poses_written(a);
    else if (name == "poses_moved") f.poses_moved();
    else if (name == "set_changes") f.set_changes();
    else if (name == "set_replaced") f.set_replaced(a != 0);
    else if (name == "set_resized") f.set_resized(a != 0);
    else if (name == "resampled_set_committed") f.resampled_set_committed();
    else if (name == "commit_rolled_back") f.commit_rolled_back();
    else if (name == "weights_touched") f.weights_touched();
    else if (name == "weights_rewrite_begins") f.weights_rewrite_begins();
    else if (name == "take_unit_weights") f.take_unit_weights();
    else if (name == "lf_sums_left") f.lf_sums_left(static_cast<uint32_t>(a));
    else if (name == "lf_sums_dropped") f.lf_sums_dropped();
    else if (name == "take_cdf_divides") f.take_cdf_divides();
    else if (name == "order_ahead_recorded") f.order_ahead_recorded(5, 1000, 2);
    else if (name == "take_order_ahead") f.take_order_ahead(5, 1000, 2);
    else if (name == "noise_ahead_recorded") f.noise_ahead_recorded(5, 1000, 64, 42);
    else if (name == "estimate_reported") f.estimate_reported(1.0, 0.0, 2.0, 3.0);
    else if (name == "nothing") {}
    else return 2;
    const FieldPosePlan plan = field_pose_plan(t, buffer, f, 1);
    std::printf("%d %d %d %d %d\n", f.field_poses_current(0) ? 1 : 0, f.field_poses_current(1) ? 1 : 0, f.field_poses_current(2) ? 1 : 0,
                plan.load ? 1 : 0, plan.rebuild_first ? 1 : 0);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("field_pose_host")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    csrc = os.path.join(ROOT, "beluga_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", csrc, "-I", os.path.join(ROOT, "include"), str(src),
                           os.path.join(csrc, "cycle_host.cpp"), "-o", str(exe)])
    return str(exe)


def play(driver, *args):
    """[(current for G = 0, 1, 2), load, rebuild first] after each event."""
    out = subprocess.check_output([driver] + list(args), text=True).splitlines()
    steps = []
    for line in out:
        v = [int(x) for x in line.split()]
        steps.append((tuple(v[:3]), v[3], v[4]) if len(v) == 5 else v[0])
    return steps


def last(driver, *args):
    return play(driver, *args)[-1]


CURRENT = ((0, 1, 0), 1, 0)  # current for generation 1 alone: the launch loads, nothing to rebuild
STALE = ((0, 0, 0), 1, 1)    # not current: the launch loads behind k_field_pose

# every transition that changes poses without writing their field-frame form
VOIDING = ["poses_moved", "set_changes", "set_replaced:0", "set_replaced:1", "set_resized:0", "set_resized:1", "resampled_set_committed",
           "commit_rolled_back"]
# ... and the ones that touch weights, sums, the order or the pivot alone
KEEPING = ["weights_touched", "weights_rewrite_begins", "take_unit_weights", "lf_sums_left:7", "lf_sums_dropped", "take_cdf_divides",
           "order_ahead_recorded", "take_order_ahead", "noise_ahead_recorded", "estimate_reported"]


def test_a_fresh_context_has_no_field_poses_and_rebuilds_first(driver):
    assert last(driver, "nothing") == STALE


def test_a_propagation_that_wrote_them_or_the_rebuild_makes_them_current_for_its_generation_alone(driver):
    assert last(driver, "field_poses_written:1") == CURRENT
    assert last(driver, "field_poses_written:0") == ((1, 0, 0), 1, 1)
    assert last(driver, "field_poses_written:2") == ((0, 0, 1), 1, 1)


@pytest.mark.parametrize("event", VOIDING)
def test_whatever_changes_poses_without_writing_them_voids_the_fact(driver, event):
    steps = play(driver, "field_poses_written:1", event, "field_poses_written:1")
    assert steps == [CURRENT, STALE, CURRENT]


@pytest.mark.parametrize("event", KEEPING)
def test_what_leaves_the_poses_alone_leaves_the_fact(driver, event):
    assert last(driver, "field_poses_written:1", event) == CURRENT


def test_a_new_map_generation_voids_it_without_an_event_of_the_set(driver):
    """mcl_set_map, the swap of a map built ahead, mcl_use_shared_map and mcl_set_likelihood_field count the context's generation up: poses
    written under generation 0 are not current for generation 1 (the plan is asked under 1), and a rebuild under 1 is."""
    steps = play(driver, "field_poses_written:0", "field_poses_written:1")
    assert steps[0] == ((1, 0, 0), 1, 1) and steps[1] == CURRENT


def test_the_steady_cycle_never_rebuilds(driver):
    """propagate (writes) -> reweight -> resample (commits) -> propagate (writes) -> reweight: the plan in front of each reweight."""
    steps = play(driver, "field_poses_written:1", "take_unit_weights", "resampled_set_committed", "field_poses_written:1", "take_unit_weights")
    assert [s[2] for s in (steps[1], steps[4])] == [0, 0] and steps[2] == STALE


def test_a_second_reweight_reuses_what_the_rebuild_left(driver):
    steps = play(driver, "set_replaced:0", "field_poses_written:1", "take_unit_weights", "nothing")
    assert steps[0] == STALE and steps[1:] == [CURRENT] * 3


def test_the_option_off_or_no_buffer_neither_loads_nor_rebuilds(driver):
    for args in (("option=0",), ("buffer=0",), ("option=0", "buffer=0")):
        assert [s[1:] for s in play(driver, *args, "nothing", "field_poses_written:1", "poses_moved")] == [(0, 0)] * 3


def test_a_propagation_stores_them_only_with_the_option_a_buffer_and_a_map(driver):
    assert play(driver, "writes:1", "writes:0") == [1, 0]
    assert play(driver, "option=0", "writes:1") == [0]
    assert play(driver, "buffer=0", "writes:1") == [0]
