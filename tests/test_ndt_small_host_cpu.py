"""The host decisions of the small NDT cycle (mcl_set_ndt_small_cycle) on the CPU, on the pattern of test_batch_beam_cpu.py: a plain
g++ compiles batch_host.cpp and cycle_host.cpp with a short driver that takes one command and its numbers (reals as C99 hex floats)
and prints what the function returned.  Which NDT members ride on the fleet's launches, where their blocks lie in the shared NDT
reweight and which member a block finds, which lone cycle is the small one, and what the host does with a cycle the tail handed back -
the recovery filters, every_n, force_update, in the order of amcl_core.hpp:179-199 - are checked against restatements written here,
without a GPU; the same driver runs once more under the address and undefined-behaviour sanitizers, as a program of its own."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
// driver <command> <numbers ...>
//   member    kind small_cycle sharded small_fused n max_particles have_map profiling    -> 0 / 1 (batch_ndt_member_fused)
//   layout    members  n[members] K[members]         -> "blocks", then a line "first_ndt blocks" per member
//   search    members  first[members]  blocks ...    -> the member of every block
//   geometry                                         -> threads, particles per block
//   small     small_cycle small_fused profiling n max_particles   -> 0 / 1 (ndt_cycle_is_small)
//   waves     small_cycle n                          -> 0 / 1 (ndt_reweight_takes_waves)
//   handback  every_n interval slow0 fast0 alpha_slow alpha_fast force  slow fast p  generator_ok
//             -> "every_n slow fast force_update" as the cycle leaves them (reals as hex floats)
#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <vector>

#include "batch_host.h"
#include "cycle_host.h"

using namespace mcl;

static char** g_arg;
static unsigned long long uword() { return std::strtoull(*g_arg++, nullptr, 0); }
static double real() { return std::strtod(*g_arg++, nullptr); }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string_view what(argv[1]);
  g_arg = argv + 2;
  char** const end = argv + argc;
  if (what == "member") {
    BatchNdtFacts m{};
    m.sensor_kind = static_cast<int>(uword());
    m.small_cycle = uword() != 0;
    m.sharded = uword() != 0;
    m.small_fused = uword() != 0;
    m.n = uword();
    m.max_particles = uword();
    m.have_map = uword() != 0;
    m.profiling = uword() != 0;
    std::printf("%d\n", batch_ndt_member_fused(m) ? 1 : 0);
  } else if (what == "layout") {
    const uint32_t members = static_cast<uint32_t>(uword());
    std::vector<uint64_t> n(members);
    std::vector<uint32_t> K(members), first(members);
    for (auto& v : n) v = uword();
    for (auto& v : K) v = static_cast<uint32_t>(uword());
    std::printf("%u\n", batch_ndt_layout(n.data(), K.data(), members, first.data()));
    for (uint32_t m = 0; m < members; ++m) std::printf("%u %u\n", first[m], batch_ndt_blocks(n[m], K[m]));
  } else if (what == "search") {
    const uint32_t members = static_cast<uint32_t>(uword());
    std::vector<uint32_t> first(members);
    for (auto& v : first) v = static_cast<uint32_t>(uword());
    while (g_arg < end) {
      const uint32_t block = static_cast<uint32_t>(uword());
      std::printf("%u\n", batch_member_of(members, block, [&](uint32_t m) { return first[m]; }));
    }
  } else if (what == "geometry") {
    std::printf("%u %u\n", kBatchNdtThreads, kBatchNdtBlock);
  } else if (what == "small") {
    NdtCycleFacts f{};
    f.small_cycle = uword() != 0;
    f.small_fused = uword() != 0;
    f.profiling = uword() != 0;
    f.n = uword();
    f.max_particles = uword();
    std::printf("%d\n", ndt_cycle_is_small(f) ? 1 : 0);
  } else if (what == "waves") {
    const bool on = uword() != 0;
    std::printf("%d\n", ndt_reweight_takes_waves(on, uword()) ? 1 : 0);
  } else if (what == "handback") {
    // the host's state in front of the cycle ...
    uint64_t every_n = uword();
    const uint64_t interval = uword();
    ExponentialFilter slow, fast;
    slow.output = real();
    fast.output = real();
    slow.alpha = real();
    fast.alpha = real();
    bool force_update = uword() != 0;
    // ... the launch of the tail stores every_n (:181 runs on the device) ...
    every_n = next_every_n(every_n, interval);
    // ... and the tail hands back: the filters' outputs as :179 leaves them, the probability
    NdtHandBack h{};
    h.slow = real();
    h.fast = real();
    h.p = real();
    const bool generator_ok = uword() != 0;
    ndt_hand_back_taken(h, slow, fast);
    if (generator_ok) ndt_hand_back_resamples(h, slow, fast, &force_update);
    std::printf("%llu %a %a %d\n", static_cast<unsigned long long>(every_n), slow.output, fast.output, force_update ? 1 : 0);
    // (the filters keep their constants: the next cycle's :179 runs with them)
    std::printf("%a %a\n", slow.alpha, fast.alpha);
  } else {
    return 2;
  }
  return 0;
}
"""


def _compile(tmp, name, extra):
    src = tmp / "driver.cpp"
    src.write_text(DRIVER)
    exe = tmp / name
    csrc = os.path.join(ROOT, "beluga_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror"] + extra +
                          ["-I", csrc, "-I", os.path.join(ROOT, "include"), str(src), os.path.join(csrc, "batch_host.cpp"),
                           os.path.join(csrc, "cycle_host.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("ndt_small_host"), "driver", [])


def _arg(v):
    return float(v).hex() if isinstance(v, float) else str(int(v))


def run(driver, what, *numbers):
    out = subprocess.check_output([driver, what] + [_arg(v) for v in numbers], text=True)
    return [[w for w in line.split()] for line in out.splitlines()]


def run_ints(driver, what, *numbers):
    return [[int(w) for w in line] for line in run(driver, what, *numbers)]


# ---- which NDT members ride on the fleet's launches ------------------------------------------------------------------------------------
LF, BEAM, LF_PROB, NDT, LANDMARK, BEARING = 0, 1, 2, 3, 4, 5
GOOD = dict(kind=NDT, small_cycle=1, sharded=0, small_fused=1, n=2000, max_particles=2000, have_map=1, profiling=0)
MEMBER_CASES = [
    (dict(), 1),
    (dict(kind=LF), 0), (dict(kind=BEAM), 0), (dict(kind=LF_PROB), 0), (dict(kind=LANDMARK), 0), (dict(kind=BEARING), 0),
    (dict(small_cycle=0), 0),
    (dict(sharded=1), 0),
    (dict(small_fused=0), 0),
    (dict(n=0), 0), (dict(n=1), 1), (dict(n=4096, max_particles=4096), 1), (dict(n=4097, max_particles=4097), 0),
    (dict(n=300, max_particles=4096), 1), (dict(n=300, max_particles=4097), 0), (dict(n=4097, max_particles=4096), 0),
    (dict(max_particles=0), 0), (dict(max_particles=1), 1),
    (dict(have_map=0), 0),
    (dict(profiling=1), 0),
]


def member_fused(m):
    """Restated from the interface's paragraph: every condition has to hold."""
    return int(m["kind"] == NDT and bool(m["small_cycle"]) and not m["sharded"] and bool(m["small_fused"]) and 1 <= m["n"] <= 4096 and
               1 <= m["max_particles"] <= 4096 and bool(m["have_map"]) and not m["profiling"])


@pytest.mark.parametrize("change,want", MEMBER_CASES)
def test_member_eligibility_every_fact_flips_alone(driver, change, want):
    m = dict(GOOD, **change)
    assert member_fused(m) == want
    got = run_ints(driver, "member", m["kind"], m["small_cycle"], m["sharded"], m["small_fused"], m["n"], m["max_particles"], m["have_map"],
                   m["profiling"])
    assert got == [[want]]


def test_geometry_restated(driver):
    """k_reweight_ndt_wave's: 256 threads, a wave of 64 per particle."""
    assert run_ints(driver, "geometry") == [[256, 256 // 64]]


# ---- prefix and grid -------------------------------------------------------------------------------------------------------------------
def layout(n, K):
    """Restated: a running sum of ceil(n / 4) over the members with particles AND measurement cells."""
    first, blocks, total = [], [], 0
    for k, c in zip(n, K):
        first.append(total)
        own = -(-k // 4) if k and c else 0
        blocks.append(own)
        total += own
    return total, list(zip(first, blocks))


FLEETS = {
    "edges_of_the_block": ([1, 4, 5, 4096], [14, 63, 64, 1]),
    "none_in_front": ([0, 7, 300], [14, 14, 3]),
    "no_cell_in_front": ([9, 7, 300], [0, 14, 3]),
    "none_in_the_middle": ([5, 0, 0, 300, 9], [14, 14, 0, 3, 65]),
    "no_cell_in_the_middle": ([5, 33, 2000, 9], [14, 0, 0, 65]),
    "none_at_the_end": ([5, 2000, 0, 0], [14, 131, 14, 0]),
    "no_cell_at_the_end": ([5, 2000, 77], [14, 131, 0]),
    "in_front_between_behind": ([0, 7, 0, 300, 9, 4096, 0, 33, 2000, 0], [14, 64, 0, 0, 65, 14, 128, 0, 1, 0]),
    "one": ([777], [14]),
    "one_without_a_block": ([777], [0]),
    "thirty_three_with_gaps": ([0 if i % 4 == 1 else 1 + 3 * i for i in range(33)], [0 if i % 7 == 3 else 14 for i in range(33)]),
    "none": ([], []),
}


@pytest.mark.parametrize("name", sorted(FLEETS))
def test_prefix_and_grid(driver, name):
    n, K = FLEETS[name]
    out = run_ints(driver, "layout", len(n), *n, *K)
    total, firsts = layout(n, K)
    assert out[0] == [total]
    assert [tuple(line) for line in out[1:]] == firsts


def test_layout_numbers_spelled_out(driver):
    n, K = FLEETS["in_front_between_behind"]
    out = run_ints(driver, "layout", len(n), *n, *K)
    assert out[0] == [2 + 3 + 1024 + 500]
    assert [line[0] for line in out[1:]] == [0, 0, 2, 2, 2, 5, 1029, 1029, 1029, 1529]


@pytest.mark.parametrize("name", [k for k in sorted(FLEETS) if layout(*FLEETS[k])[0]])
def test_search_finds_the_member_of_every_block(driver, name):
    n, K = FLEETS[name]
    total, firsts = layout(n, K)
    want = [m for m, (_, own) in enumerate(firsts) for _ in range(own)]
    assert len(want) == total
    got = run_ints(driver, "search", len(n), *[f for f, _ in firsts], *range(total))
    assert [g[0] for g in got] == want
    assert all(n[m] and K[m] for m in want)  # a member with n = 0 or K = 0 is never found


# ---- is this NDT cycle a small one -------------------------------------------------------------------------------------------------------
SMALL_CASES = [
    (dict(), 1),
    (dict(small_cycle=0), 0), (dict(small_fused=0), 0), (dict(profiling=1), 0),
    (dict(n=4096, max_particles=4096), 1), (dict(n=4097, max_particles=4096), 0), (dict(n=4096, max_particles=4097), 0),
    (dict(n=4097, max_particles=4097), 0), (dict(n=500, max_particles=4096), 1), (dict(n=500, max_particles=4097), 0),
    (dict(n=1, max_particles=1), 1), (dict(n=0), 0), (dict(max_particles=0), 0),
]


@pytest.mark.parametrize("change,want", SMALL_CASES)
def test_small_cycle_predicate(driver, change, want):
    f = dict(dict(small_cycle=1, small_fused=1, profiling=0, n=2000, max_particles=2000), **change)
    restated = int(bool(f["small_cycle"]) and bool(f["small_fused"]) and not f["profiling"] and 1 <= f["n"] <= 4096 and
                   1 <= f["max_particles"] <= 4096)
    assert restated == want
    assert run_ints(driver, "small", f["small_cycle"], f["small_fused"], f["profiling"], f["n"], f["max_particles"]) == [[want]]


@pytest.mark.parametrize("on,n,want", [(1, 1, 1), (1, 4096, 1), (1, 4097, 0), (0, 1, 0), (0, 4096, 0), (1, 0, 1)])
def test_stage_level_reweight_takes_the_wave_kernel(driver, on, n, want):
    assert run_ints(driver, "waves", on, n) == [[want]]


# ---- what follows a hand-back ------------------------------------------------------------------------------------------------------------
def thrun(slow, fast, a_slow, a_fast, average):
    """thrun_recovery_probability_estimator.hpp:69-89 over exponential_filter.hpp:32-44: the outputs and the probability."""
    fast = fast + (average if fast == 0.0 else a_fast * (average - fast))
    slow = slow + (average if slow == 0.0 else a_slow * (average - slow))
    p = min(max(1.0 - fast / slow, 0.0), 1.0) if abs(slow) >= 2.220446049250313e-16 else 0.0
    return slow, fast, p


@pytest.mark.parametrize("generator_ok", [1, 0])
@pytest.mark.parametrize("every_n,interval", [(0, 1), (0, 3), (1, 3), (2, 3)])
@pytest.mark.parametrize("force", [0, 1])
def test_hand_back_bookkeeping_follows_the_reference_order(driver, generator_ok, every_n, interval, force):
    """amcl_core.hpp:179-199 for a cycle that resamples with p > 0: :179 the estimator advances, :181 every_n counts, :182 the generator
    (may throw), :184-186 the reset, :188 the draw, :199 force_update cleared.  A throw at :182 leaves 179 and 181 done and nothing else."""
    a_slow, a_fast = 0.001, 0.1
    slow0, fast0 = 2.0 / 2000, 0.5 / 2000
    slow, fast, p = thrun(slow0, fast0, a_slow, a_fast, 1.0 / 2000)
    assert p > 0.0
    out = run(driver, "handback", every_n, interval, slow0, fast0, a_slow, a_fast, force, slow, fast, p, generator_ok)
    got_every_n, got_slow, got_fast, got_force = int(out[0][0]), float.fromhex(out[0][1]), float.fromhex(out[0][2]), int(out[0][3])
    assert got_every_n == (every_n + 1) % interval
    if generator_ok:
        assert (got_slow, got_fast, got_force) == (0.0, 0.0, 0)
    else:
        assert (got_slow, got_fast, got_force) == (slow, fast, force)
    assert [float.fromhex(v) for v in out[1]] == [a_slow, a_fast]


def test_hand_back_reset_is_the_probabilitys(driver):
    """The reset of :184-186 belongs to p > 0 - what every handed-back cycle has; the function still asks."""
    out = run(driver, "handback", 0, 1, 0.25, 0.5, 0.001, 0.1, 1, 0.125, 0.375, 0.0, 1)
    assert [float.fromhex(out[0][1]), float.fromhex(out[0][2]), int(out[0][3])] == [0.125, 0.375, 0]


# ---- the same driver under the sanitizers, as a program of its own ---------------------------------------------------------------------------
def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = _compile(tmp_path, "driver_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    n, K = FLEETS["thirty_three_with_gaps"]
    total, firsts = layout(n, K)
    for args in (["layout", len(n), *n, *K], ["layout", 0], ["layout", 1, 777, 0], ["search", len(n), *[f for f, _ in firsts], *range(total)],
                 ["search", 1, 0, 0, 5], ["member", NDT, 1, 0, 1, 2000, 2000, 1, 0], ["small", 1, 1, 0, 4096, 4097], ["waves", 1, 4096],
                 ["handback", 2, 3, 0.001, 0.00025, 0.001, 0.1, 1, 0.00099, 0.000275, 0.72, 1],
                 ["handback", 2, 3, 0.001, 0.00025, 0.001, 0.1, 1, 0.00099, 0.000275, 0.72, 0], ["geometry"]):
        done = subprocess.run([exe, args[0]] + [_arg(a) for a in args[1:]], capture_output=True, text=True)
        assert done.returncode == 0 and "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr, (args, done.stderr)


# ---- header and bindings ---------------------------------------------------------------------------------------------------------------------
def test_header_and_bindings_name_the_calls():
    from beluga_amd import capi
    text = open(os.path.join(ROOT, "include", "beluga_mcl.h")).read()
    for word in ("mcl_set_ndt_small_cycle", "mcl_get_ndt_small_cycle", "mcl_get_ndt_small_cycle_counts", "mcl_ndt_batch_counts"):
        assert re.search(r"\b" + word + r"\b", text), word
        assert word in capi.exported_names()
