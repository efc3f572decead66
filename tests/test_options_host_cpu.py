"""The table of the per-context switches (beluga_amd/csrc/options_host.cpp) on the CPU: a plain g++ compiles the file with a short
driver.  The option names are pinned here - they are public strings - and what set_tuning stores for every name and probe value is
compared with tests/golden/options_parent_values.txt: what the if-chain of mcl_set_option stored before the table took its place,
recorded from that chain itself and not from the table."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OPTION_NAMES = [
    "lf_variant", "lf_fast", "lf_table", "lf_patch", "lf_dispersed", "lf_far_tiles", "key_layout", "lf_loose_below", "lf_small_particles",
    "device_policy", "sort_min_particles", "beam_sort_min_particles", "field_build", "key_curve", "key_warp", "key_bits_xy", "lf_margin",
    "lf_split", "lf_queue_grid", "shard_pad_permille", "lf_queue", "lf_ends_first", "beam_free_ahead", "beam_sectors", "lf_weight_sums",
    "beam_table", "cycle_spin", "scan_fused", "draw_fold", "lf_unit_weights", "small_fused", "norm_store", "noise_ahead", "order_ahead",
    "lf_far_beams_per_wave", "batch_cluster_fused", "batch_beam_fused", "draw_key_hist", "rows_merged"]

PROBES = [-2**40, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 224, 257, 258, 4096, 4097, 8000, 8001, 2**20, 2**20 + 1, 2**30, 2**30 + 1, 2**31 - 1, 2**31,
          2**40]

DRIVER = r"""
// driver names                      -> the table's names, one per line
// driver set <name> <values ...>    -> per value: accepted (0 / 1), the member called <name> afterwards, members that differ from the defaults
// driver env <VAR=text ...>         -> "lookup <variable>" per look-up, then "<name> <member>" per pinned name
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "options_host.h"

using namespace mcl;

// the test's own idea of which member a name means: the member of that name
struct Member { const char* name; int Tuning::*member; };
static const Member kMembers[] = {@MEMBERS@};

static int differing(const Tuning& a, const Tuning& b) {
  static_assert(sizeof(Tuning) % sizeof(int) == 0, "Tuning is a row of ints");
  int av[sizeof(Tuning) / sizeof(int)], bv[sizeof(Tuning) / sizeof(int)];
  std::memcpy(av, &a, sizeof a);
  std::memcpy(bv, &b, sizeof b);
  int count = 0;
  for (size_t i = 0; i < sizeof(Tuning) / sizeof(int); ++i) count += av[i] != bv[i];
  return count;
}

int main(int argc, char** argv) {
  const std::string what = argc > 1 ? argv[1] : "";
  if (what == "names") {
    size_t count = 0;
    const char* const* names = tuning_names(&count);
    for (size_t i = 0; i < count; ++i) std::printf("%s\n", names[i]);
    return 0;
  }
  if (what == "set") {
    const char* name = argv[2];
    int Tuning::*member = nullptr;
    for (const Member& m : kMembers)
      if (std::strcmp(m.name, name) == 0) member = m.member;
    for (int i = 3; i < argc; ++i) {
      Tuning t;
      const bool ok = set_tuning(t, name, std::strtoll(argv[i], nullptr, 10));
      std::printf("%d %d %d\n", ok ? 1 : 0, member ? t.*member : 0, differing(t, Tuning{}));
    }
    return 0;
  }
  if (what == "env") {
    std::vector<std::pair<std::string, std::string>> vars;
    for (int i = 2; i < argc; ++i) {
      const std::string a = argv[i];
      vars.emplace_back(a.substr(0, a.find('=')), a.substr(a.find('=') + 1));
    }
    Tuning t;
    tuning_from_environment(t, [&](const char* name) -> const char* {
      std::printf("lookup %s\n", name);
      for (const auto& v : vars)
        if (v.first == name) return v.second.c_str();
      return nullptr;
    });
    for (const Member& m : kMembers) std::printf("%s %d\n", m.name, t.*m.member);
    return 0;
  }
  return 2;
}
"""


def driver_source():
    return DRIVER.replace("@MEMBERS@", ", ".join('{"%s", &Tuning::%s}' % (n, n) for n in OPTION_NAMES))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("options_host")
    src = d / "driver.cpp"
    src.write_text(driver_source())
    exe = d / "driver"
    csrc = os.path.join(ROOT, "beluga_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", csrc, str(src), os.path.join(csrc, "options_host.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def parent_values():
    table = {}
    with open(os.path.join(ROOT, "tests", "golden", "options_parent_values.txt")) as f:
        rows = [line.split() for line in f if line.strip() and not line.startswith("#")]
    assert rows[0][0] == "probes"
    probes = [int(v) for v in rows[0][1:]]
    for name, *stored in rows[1:]:
        assert len(stored) == len(probes)
        table.update({(name, p): int(v) for p, v in zip(probes, stored)})
    return table


@pytest.fixture(scope="module")
def defaults(driver):
    out = subprocess.check_output([driver, "env"], text=True).splitlines()
    return {name: int(v) for name, v in (line.split() for line in out if not line.startswith("lookup "))}


def test_option_names_are_the_pinned_ones(driver):
    assert len(OPTION_NAMES) == 39 and len(set(OPTION_NAMES)) == 39
    assert subprocess.check_output([driver, "names"], text=True).split() == OPTION_NAMES


def test_recorded_table_covers_every_name_and_probe(parent_values):
    assert sorted(parent_values) == sorted((n, p) for n in OPTION_NAMES for p in PROBES)


def test_stored_values_are_the_if_chains(driver, parent_values, defaults):
    for name in OPTION_NAMES:
        out = subprocess.check_output([driver, "set", name] + [str(p) for p in PROBES], text=True).splitlines()
        assert len(out) == len(PROBES)
        for probe, line in zip(PROBES, out):
            ok, stored, changed = map(int, line.split())
            want = parent_values[(name, probe)]
            assert ok == 1, (name, probe)
            assert stored == want, (name, probe, stored, want)
            # no other member moves: the members that differ from the defaults are this one, if it does
            assert changed == (1 if want != defaults[name] else 0), (name, probe, changed)


def test_unknown_name_is_refused_and_changes_nothing(driver):
    for name in ["no_such_option", "", "lf_variant ", "LF_VARIANT", "device_cus"]:
        out = subprocess.check_output([driver, "set", name, "1", "0", "-1"], text=True).splitlines()
        assert [line.split()[0::2] for line in out] == [["0", "0"]] * 3, name


def test_environment_reads_exactly_the_tables_variables(driver, defaults):
    out = subprocess.check_output([driver, "env"], text=True).splitlines()
    assert [line.split()[1] for line in out if line.startswith("lookup ")] == ["BELUGA_MCL_" + n.upper() for n in OPTION_NAMES]
    # a variable for a name that is no option is not looked up; an unset variable leaves the default
    out = subprocess.check_output([driver, "env", "BELUGA_MCL_DEVICE_CUS=7", "BELUGA_MCL_NO_SUCH=1", "BELUGA_MCL_LF_TABLE=cube",
                                   "BELUGA_MCL_KEY_BITS_XY=5", "BELUGA_MCL_LF_PATCH=9", "BELUGA_MCL_SHARD_PAD_PERMILLE=9000",
                                   "BELUGA_MCL_CYCLE_SPIN=-3", "BELUGA_MCL_LF_FAST=zero"], text=True).splitlines()
    looked_up = [line.split()[1] for line in out if line.startswith("lookup ")]
    assert "BELUGA_MCL_DEVICE_CUS" not in looked_up and "BELUGA_MCL_NO_SUCH" not in looked_up and len(looked_up) == 39
    got = {name: int(v) for name, v in (line.split() for line in out if not line.startswith("lookup "))}
    want = dict(defaults, lf_table=1, key_bits_xy=5, lf_patch=1, shard_pad_permille=8000, cycle_spin=-1, lf_fast=0)  # (atoi("zero") = 0)
    assert got == want
    out = subprocess.check_output([driver, "env", "BELUGA_MCL_LF_TABLE=0"], text=True).splitlines()
    assert dict(line.split() for line in out if not line.startswith("lookup "))["lf_table"] == "0"
