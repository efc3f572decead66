"""Beam skipping on the CPU: the decision rule, the level and the parameter checks of beluga_amd/csrc/beam_skip_host.cpp - a plain g++
compiles the file with a short driver - against tests/beam_skip_reference.py, the edges of the rule included; the ABI's struct sizes,
offsets and defaults through beluga_amd/capi.py; the batch's fused test saying no to a member with skipping on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import beam_skip_reference as bref
from beluga_amd import build as mcl_build
from beluga_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beluga_amd", "csrc")

DRIVER = r"""
// driver decide <n> <threshold> <error_threshold> <counts ...>  -> "<kept as 0/1 string or -> <skipped> <used_all>"
// driver level <z_hit> <z_random> <sigma_hit> <max_laser_distance> <distance>  -> the float's bits
// driver check <enabled> <distance> <threshold> <error_threshold>  -> 1 (fine) / 0
// driver abi  -> sizes and offsets of the two structs
// driver fused <beam_skip>  -> batch_member_fused of an otherwise fused member
// (doubles come as C99 hex floats)
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "batch_host.h"
#include "beam_skip_host.h"

using namespace mcl;

int main(int argc, char** argv) {
  const std::string what = argc > 1 ? argv[1] : "";
  auto d = [&](int i) { return std::strtod(argv[i], nullptr); };
  if (what == "decide") {
    const uint64_t n = std::strtoull(argv[2], nullptr, 10);
    std::vector<uint32_t> counts;
    for (int i = 5; i < argc; ++i) counts.push_back(static_cast<uint32_t>(std::strtoul(argv[i], nullptr, 10)));
    std::vector<uint8_t> kept(counts.size() + 1, 7);
    const BeamSkipDecision r = beam_skip_decide(counts.data(), counts.size(), n, d(3), d(4), kept.data());
    const BeamSkipDecision again = beam_skip_decide(counts.data(), counts.size(), n, d(3), d(4), nullptr);
    if (again.skipped != r.skipped || again.used_all != r.used_all || kept[counts.size()] != 7) return 2;
    std::string mask = "-";
    for (size_t b = 0; b < counts.size(); ++b) mask += kept[b] ? '1' : '0';
    std::printf("%s %llu %d\n", mask.c_str(), static_cast<unsigned long long>(r.skipped), r.used_all ? 1 : 0);
    return 0;
  }
  if (what == "level") {
    mcl_lf_params lf{};
    lf.z_hit = d(2), lf.z_random = d(3), lf.sigma_hit = d(4), lf.max_laser_distance = d(5);
    const float v = beam_skip_level(lf, d(6));
    uint32_t bits;
    std::memcpy(&bits, &v, sizeof bits);
    std::printf("%u\n", bits);
    return 0;
  }
  if (what == "check") {
    const mcl_beam_skip_params p{static_cast<int32_t>(std::strtol(argv[2], nullptr, 10)), 0, d(3), d(4), d(5)};
    std::printf("%d\n", beam_skip_check_params(p) == nullptr ? 1 : 0);
    return 0;
  }
  if (what == "abi") {
    std::printf("%zu %zu %zu %zu %zu\n", sizeof(mcl_beam_skip_params), offsetof(mcl_beam_skip_params, enabled), offsetof(mcl_beam_skip_params, distance),
                offsetof(mcl_beam_skip_params, threshold), offsetof(mcl_beam_skip_params, error_threshold));
    std::printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(mcl_beam_skip_result), offsetof(mcl_beam_skip_result, valid), offsetof(mcl_beam_skip_result, used_all),
                offsetof(mcl_beam_skip_result, num_beams), offsetof(mcl_beam_skip_result, num_particles), offsetof(mcl_beam_skip_result, num_skipped),
                offsetof(mcl_beam_skip_result, level));
    return 0;
  }
  if (what == "fused") {
    BatchMemberFacts m{};
    m.sensor_kind = MCL_SENSOR_LIKELIHOOD_FIELD, m.small_fused = true, m.n = 1000, m.max_particles = 2000, m.palette_beams = true;
    m.beam_skip = std::strtol(argv[2], nullptr, 10) != 0;
    std::printf("%d\n", batch_member_fused(m) ? 1 : 0);
    return 0;
  }
  return 1;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("beam_skip_host")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src),
                           os.path.join(CSRC, "beam_skip_host.cpp"), os.path.join(CSRC, "batch_host.cpp"), "-o", str(exe)])

    def run(*args):
        return subprocess.check_output([str(exe)] + [a if isinstance(a, str) else (float(a).hex() if isinstance(a, float) else str(a)) for a in args],
                                       text=True).split("\n")[:-1]
    return run


def host_decide(driver, counts, n, params):
    mask, skipped, used_all = driver("decide", int(n), float(params["threshold"]), float(params["error_threshold"]), *[int(c) for c in counts])[0].split()
    return np.array([c == "1" for c in mask[1:]], dtype=bool), int(skipped), bool(int(used_all))


def check_decide(driver, counts, n, threshold, error_threshold):
    params = dict(bref.DEFAULTS, threshold=threshold, error_threshold=error_threshold)
    kept, skipped, used_all = host_decide(driver, counts, n, params)
    want_kept, want_skipped, want_all = bref.decide(counts, n, len(counts), params)
    assert np.array_equal(kept, want_kept) and skipped == want_skipped and used_all == want_all, (counts, n, threshold, error_threshold)
    return kept, skipped, used_all


def test_decision_rule_matches_the_reference_on_random_votes(driver):
    rng = np.random.Generator(np.random.MT19937(5))
    for _ in range(60):
        n = int(rng.integers(1, 5000))
        B = int(rng.integers(1, 200))
        counts = rng.integers(0, n + 1, B)
        check_decide(driver, counts, n, float(rng.choice([0.0, 0.1, 0.3, 0.5, 0.9, 1.0, rng.uniform()])),
                     float(rng.choice([0.0, 0.5, 0.9, 1.0, rng.uniform()])))


def test_a_share_equal_to_the_threshold_is_not_kept(driver):
    # 0.25 = 500 / 2000 = 1 / 4 exactly: equal is not greater; one particle more is
    kept, skipped, _ = check_decide(driver, [500, 501, 499], 2000, 0.25, 0.9)
    assert kept.tolist() == [False, True, False] and skipped == 2
    # 0.3 is no binary fraction: 3 / 10 rounds to the same double as the literal, so it is equal there too
    assert 3.0 / 10.0 == 0.3
    kept, _, _ = check_decide(driver, [3, 4], 10, 0.3, 1.0)
    assert kept.tolist() == [False, True]


def test_a_skipped_share_equal_to_the_error_threshold_uses_all(driver):
    # 9 of 10 skipped: 9.0 / 10.0 == 0.9 as doubles - all used; 8 of 10 not
    assert 9.0 / 10.0 == 0.9
    _, skipped, used_all = check_decide(driver, [0] * 9 + [10], 10, 0.3, 0.9)
    assert skipped == 9 and used_all
    _, skipped, used_all = check_decide(driver, [0] * 8 + [10, 10], 10, 0.3, 0.9)
    assert skipped == 8 and not used_all
    # 3 of 4 at 0.75
    _, _, used_all = check_decide(driver, [0, 0, 0, 4], 4, 0.5, 0.75)
    assert used_all


def test_thresholds_zero_and_one(driver):
    # threshold 0: a beam with one vote is kept, one with none is not; threshold 1: nothing exceeds it, everything is skipped -> all used
    kept, skipped, used_all = check_decide(driver, [0, 1, 7], 7, 0.0, 0.9)
    assert kept.tolist() == [False, True, True] and skipped == 1 and not used_all
    kept, skipped, used_all = check_decide(driver, [7, 7, 7], 7, 1.0, 0.9)
    assert not kept.any() and skipped == 3 and used_all
    # error_threshold 0: 0 / B >= 0 - every scan is used whole; error_threshold 1: only a scan with every beam skipped
    assert check_decide(driver, [7, 7], 7, 0.3, 0.0)[2]
    assert not check_decide(driver, [7, 0], 7, 0.3, 1.0)[2]
    assert check_decide(driver, [0, 0], 7, 0.3, 1.0)[2]


def test_no_beams_and_one_particle(driver):
    kept, skipped, used_all = check_decide(driver, [], 100, 0.3, 0.0)
    assert len(kept) == 0 and skipped == 0 and not used_all  # B == 0: never "all used"
    kept, skipped, used_all = check_decide(driver, [1, 0, 1, 1], 1, 0.3, 0.9)
    assert kept.tolist() == [True, False, True, True] and skipped == 1 and not used_all


@pytest.mark.parametrize("lf", [(0.5, 0.5, 0.2, 2.0), (0.5, 0.5, 0.2, 100.0), (0.95, 0.05, 0.05, 30.0), (1.0, 0.0, 1.0, 12.0)])
def test_level_is_the_field_builders_expression(driver, lf):
    for distance in (0.05, 0.17, 0.5, 1.0, 3.7, 1e-3, 50.0):
        got = np.array([int(driver("level", *[float(v) for v in lf], float(distance))[0])], dtype=np.uint32).view(np.float32)[0]
        want = bref.level(*lf, distance)
        assert abs(int(got.view(np.uint32)) - int(want.view(np.uint32))) <= 1, (lf, distance, got, want)  # one float ulp: exp's last bit
        assert got >= np.float32(lf[1] / lf[3]) - np.float32(1e-9)


def test_parameter_checks(driver):
    ok = lambda *p: driver("check", *p)[0] == "1"
    assert ok(0, 0.5, 0.3, 0.9) and ok(1, 0.5, 0.3, 0.9) and ok(1, 1e-9, 0.0, 1.0) and ok(1, 1e9, 1.0, 0.0)
    for bad in ((2, 0.5, 0.3, 0.9), (-1, 0.5, 0.3, 0.9), (1, 0.0, 0.3, 0.9), (1, -0.5, 0.3, 0.9), (1, float("inf"), 0.3, 0.9),
                (1, float("nan"), 0.3, 0.9), (1, 0.5, -1e-9, 0.9), (1, 0.5, 1.0000001, 0.9), (1, 0.5, float("nan"), 0.9),
                (1, 0.5, 0.3, -0.1), (1, 0.5, 0.3, 1.5), (1, 0.5, 0.3, float("nan")), (1, 0.5, float("inf"), 0.9)):
        assert not ok(*bad), bad


def test_a_member_with_skipping_on_is_not_fused(driver):
    assert driver("fused", 0)[0] == "1" and driver("fused", 1)[0] == "0"


def test_abi_structs_defaults_and_symbols(driver):
    params_line, result_line = (list(map(int, line.split())) for line in driver("abi"))
    P, R = capi.BeamSkipParams, capi.BeamSkipResult
    assert params_line == [C.sizeof(P), P.enabled.offset, P.distance.offset, P.threshold.offset, P.error_threshold.offset] == [32, 0, 8, 16, 24]
    assert result_line == [C.sizeof(R), R.valid.offset, R.used_all.offset, R.num_beams.offset, R.num_particles.offset, R.num_skipped.offset,
                           R.level.offset] == [40, 0, 4, 8, 16, 24, 32]
    mcl_build.build()
    lib = capi.load()
    p = P(9, 9, 9.0, 9.0, 9.0)
    lib.mcl_default_beam_skip_params(C.byref(p))
    assert (p.enabled, p.reserved0, p.distance, p.threshold, p.error_threshold) == (0, 0, 0.5, 0.3, 0.9)
    assert {k: getattr(p, k) for k in bref.DEFAULTS} == bref.DEFAULTS
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "beluga_mcl.h")).read(), flags=re.S)
    for name in ("mcl_set_beam_skip", "mcl_get_beam_skip", "mcl_get_beam_skip_result", "mcl_beam_agreement"):
        assert re.search(r"\bmcl_status\s+" + name + r"\s*\(", header), f"{name} is not declared in beluga_mcl.h"
        assert hasattr(lib, name) and name in capi.exported_names()
    assert re.search(r"\bvoid\s+mcl_default_beam_skip_params\s*\(", header)
