"""The cached facts about the live particle set (beluga_amd/csrc/set_facts.h) on the CPU: a plain g++ compiles the header with a
short driver that plays a sequence of events and prints, after each one, what the event returned and what the facts say - read
non-destructively, through takes on a copy.  The assertions are the event x fact table of the header."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
// driver event[:a,b,c,d] ...   One line per event: <returned> <unit> <lf sums> <divides> <order recorded> <order accepted> <normals' n>
// (returned: the take's value, recorded + 2 * matched for take_order, - for an event that returns nothing).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "set_facts.h"

using mcl::SetFacts;

int main(int argc, char** argv) {
  SetFacts f;
  for (int k = 1; k < argc; ++k) {
    std::string name(argv[k]);
    unsigned long long a[4] = {0, 0, 0, 0};
    if (const size_t colon = name.find(':'); colon != std::string::npos) {
      const char* p = argv[k] + colon + 1;
      for (int j = 0; j < 4 && *p; ++j) {
        char* end = nullptr;
        a[j] = std::strtoull(p, &end, 10);
        p = *end ? end + 1 : end;
      }
      name.resize(colon);
    }
    long long ret = -1;
    if (name == "set_changes") f.set_changes();
    else if (name == "set_replaced") f.set_replaced(a[0] != 0);
    else if (name == "set_resized") f.set_resized(a[0] != 0);
    else if (name == "weights_rewrite_begins") f.weights_rewrite_begins();
    else if (name == "weights_touched") f.weights_touched();
    else if (name == "take_unit_weights") ret = f.take_unit_weights();
    else if (name == "lf_sums_left") f.lf_sums_left(static_cast<uint32_t>(a[0]));
    else if (name == "lf_sums_dropped") f.lf_sums_dropped();
    else if (name == "weights_left_undivided") f.weights_left_undivided(a[0] != 0);
    else if (name == "take_cdf_divides") ret = f.take_cdf_divides();
    else if (name == "resampled_set_committed") f.resampled_set_committed();
    else if (name == "commit_rolled_back") f.commit_rolled_back();
    else if (name == "order_ahead_recorded") f.order_ahead_recorded(static_cast<uint32_t>(a[0]), a[1], static_cast<uint32_t>(a[2]));
    else if (name == "take_order_ahead") {
      const SetFacts::OrderTaken t = f.take_order_ahead(static_cast<uint32_t>(a[0]), a[1], static_cast<uint32_t>(a[2]));
      ret = (t.recorded ? 1 : 0) + (t.matched ? 2 : 0);
    } else if (name == "order_accepted") f.order_accepted(a[0] != 0);
    else if (name == "take_order_accepted") ret = f.take_order_accepted();
    else if (name == "noise_ahead_recorded") f.noise_ahead_recorded(static_cast<uint32_t>(a[0]), a[1], a[2], a[3]);
    else if (name == "noise_ahead_serves") ret = f.noise_ahead_serves(static_cast<uint32_t>(a[0]), a[1], a[2], a[3]);  // (step, n, seed, offset)
    else return 2;
    SetFacts divides = f, order = f, accepted = f;
    if (ret < 0) std::printf("-");
    else std::printf("%lld", ret);
    std::printf(" %d %u %d %d %d %llu\n", f.unit_weights() ? 1 : 0, f.lf_sums(), divides.take_cdf_divides() ? 1 : 0,
                order.take_order_ahead(0, 0, 0).recorded ? 1 : 0, accepted.take_order_accepted() ? 1 : 0,
                static_cast<unsigned long long>(f.noise_ahead_count()));
  }
  return 0;
}
"""

FIELDS = ("unit", "lf_sums", "divides", "order", "accepted", "normals")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("set_facts")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "beluga_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


def play(driver, *events):
    """[(returned or None, {fact: value})] after each event."""
    out = subprocess.check_output([driver] + list(events), text=True).splitlines()
    assert len(out) == len(events)
    steps = []
    for line in out:
        words = line.split()
        steps.append((None if words[0] == "-" else int(words[0]), dict(zip(FIELDS, map(int, words[1:])))))
    return steps


def last(driver, *events):
    return play(driver, *events)[-1]


# Every fact standing at once: unit weights, 7 LF sums, undivided weights, an order for (5, 1000, 2) that was accepted, normals for (5, 1000, offset 64, seed 42).
FULL = ("resampled_set_committed", "lf_sums_left:7", "weights_left_undivided:1", "order_ahead_recorded:5,1000,2", "order_accepted:1",
        "noise_ahead_recorded:5,1000,64,42")
FULL_STATE = dict(unit=1, lf_sums=7, divides=1, order=1, accepted=1, normals=1000)


def test_a_fresh_context_knows_nothing(driver):
    assert last(driver, "noise_ahead_serves:0,1,0,0") == (0, dict(unit=0, lf_sums=0, divides=0, order=0, accepted=0, normals=0))
    assert last(driver, *FULL)[1] == FULL_STATE


@pytest.mark.parametrize("event", ["set_replaced:1", "resampled_set_committed"])
@pytest.mark.parametrize("before", [(), ("weights_touched",), ("weights_rewrite_begins",), ("commit_rolled_back",)])
def test_every_all_ones_event_sets_the_unit_flag(driver, event, before):
    assert last(driver, *before, event)[1]["unit"] == 1


@pytest.mark.parametrize("event", ["weights_touched", "weights_rewrite_begins", "set_replaced:0", "set_resized:1", "commit_rolled_back",
                                   "take_unit_weights"])
def test_every_weight_touching_event_clears_the_unit_flag_and_nothing_else_of_its_own(driver, event):
    _, state = last(driver, *FULL, event)
    voided = dict(lf_sums=0, order=0) if event.startswith("set_") else {}
    assert state == {**FULL_STATE, "unit": 0, **voided}


def test_a_rewrite_that_begins_and_never_succeeds_leaves_the_unit_flag_false(driver):
    steps = play(driver, "set_replaced:1", "set_changes", "weights_rewrite_begins", "take_unit_weights")
    assert [s[1]["unit"] for s in steps] == [1, 1, 0, 0] and steps[-1][0] == 0
    # ... and one that succeeds installs the set with it
    assert last(driver, "set_changes", "weights_rewrite_begins", "set_replaced:1")[1]["unit"] == 1


def test_the_reweight_takes_the_unit_flag_once(driver):
    steps = play(driver, "resampled_set_committed", "take_unit_weights", "take_unit_weights")
    assert [s[0] for s in steps[1:]] == [1, 0] and [s[1]["unit"] for s in steps] == [1, 0, 0]


@pytest.mark.parametrize("events", [("set_changes",), ("set_replaced:0",), ("set_replaced:1",), ("set_resized:0",), ("set_resized:1",),
                                    ("lf_sums_dropped", "resampled_set_committed")])
def test_lf_sums_do_not_outlive_the_set_they_describe(driver, events):
    """(the last one: do_resample drops them where it begins, and commits at its end)"""
    assert last(driver, "lf_sums_left:12")[1]["lf_sums"] == 12
    assert last(driver, "lf_sums_left:12", *events)[1]["lf_sums"] == 0


def test_lf_sums_are_consumed_once_and_only_by_dropping(driver):
    steps = play(driver, *FULL, "weights_touched", "take_cdf_divides", "lf_sums_dropped", "lf_sums_dropped")
    assert [s[1]["lf_sums"] for s in steps[len(FULL):]] == [7, 7, 0, 0]
    assert steps[-1][1] == {**FULL_STATE, "unit": 0, "divides": 0, "lf_sums": 0}


def test_undivided_weights_are_taken_once_by_the_cdf(driver):
    steps = play(driver, "weights_left_undivided:1", "take_cdf_divides", "take_cdf_divides", "weights_left_undivided:1", "weights_left_undivided:0",
                 "take_cdf_divides")
    assert [s[0] for s in steps] == [None, 1, 0, None, None, 0]
    assert [s[1]["divides"] for s in steps] == [1, 0, 0, 1, 0, 0]


def test_an_order_ahead_is_taken_once(driver):
    steps = play(driver, "order_ahead_recorded:5,1000,2", "take_order_ahead:5,1000,2", "take_order_ahead:5,1000,2")
    assert [s[0] for s in steps[1:]] == [3, 0]  # recorded and matched; then no record
    assert [s[1]["order"] for s in steps] == [1, 0, 0]
    assert last(driver, "take_order_ahead:0,0,0")[0] == 0  # (a fresh context's zeros are no record of step 0)


@pytest.mark.parametrize("other", ["6,1000,2", "5,999,2", "5,1001,2", "5,1000,3"])
def test_an_order_ahead_for_another_step_size_or_layout_is_refused_and_still_consumed(driver, other):
    steps = play(driver, "order_ahead_recorded:5,1000,2", "take_order_ahead:" + other, "take_order_ahead:5,1000,2")
    assert [s[0] for s in steps[1:]] == [1, 0]  # a record, no match; then no record
    assert steps[1][1]["order"] == 0


@pytest.mark.parametrize("event", ["set_changes", "set_replaced:1", "set_resized:0"])
def test_an_order_ahead_does_not_outlive_the_set(driver, event):
    assert last(driver, "order_ahead_recorded:5,1000,2", event, "take_order_ahead:5,1000,2")[0] == 0


def test_the_accepted_order_is_handed_to_one_reweight(driver):
    steps = play(driver, "order_accepted:1", "take_order_accepted", "take_order_accepted", "order_accepted:1", "order_accepted:0", "take_order_accepted")
    assert [s[0] for s in steps] == [None, 1, 0, None, None, 0]


def test_normals_ahead_serve_their_step_seed_and_offset_up_to_their_count(driver):
    rec = "noise_ahead_recorded:5,1000,64,42"  # (step, n, offset, seed); serves: (step, n, seed, offset)
    for n in (1, 999, 1000):
        assert last(driver, rec, "noise_ahead_serves:5,%d,42,64" % n)[0] == 1
    for other in ("5,1001,42,64", "4,1000,42,64", "6,1000,42,64", "5,1000,43,64", "5,1000,42,0", "5,1000,64,42"):
        assert last(driver, rec, "noise_ahead_serves:" + other)[0] == 0
    assert last(driver, rec)[1]["normals"] == 1000


@pytest.mark.parametrize("event", ["set_changes", "set_replaced:0", "set_replaced:1", "set_resized:1", "resampled_set_committed", "commit_rolled_back",
                                   "weights_touched"])
def test_normals_ahead_survive_whatever_happens_to_the_set(driver, event):
    assert last(driver, "noise_ahead_recorded:5,1000,64,42", event, "noise_ahead_serves:5,1000,42,64")[0] == 1


def test_a_rollback_puts_the_old_sets_weights_back_and_leaves_the_rest_as_the_commit_left_it(driver):
    steps = play(driver, *FULL, "weights_touched", "resampled_set_committed", "commit_rolled_back")
    committed, rolled_back = steps[-2][1], steps[-1][1]
    assert committed == FULL_STATE
    assert rolled_back == {**committed, "unit": 0}


def test_shrinking_keeps_the_unit_flag_and_growing_clears_it(driver):
    assert last(driver, *FULL, "set_resized:0")[1] == {**FULL_STATE, "lf_sums": 0, "order": 0}
    assert last(driver, *FULL, "set_resized:1")[1] == {**FULL_STATE, "lf_sums": 0, "order": 0, "unit": 0}
    assert last(driver, "weights_touched", "set_resized:0")[1]["unit"] == 0  # (shrinking makes no weight 1.0)
