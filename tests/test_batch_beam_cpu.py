"""The arithmetic of a batch's beam-model members (beluga_amd/csrc/batch_host.cpp) on the CPU, on the pattern of test_batch_cpu.py: a
plain g++ compiles the file with a short driver that takes one command and its numbers and prints what the function returned.  Which
beam members ride on the fleet's launches, where their blocks lie in the shared beam reweight, how much workgroup memory it needs and
the block-to-member search over that prefix are checked against restatements written here, without a GPU; the same driver runs once
more under the address and undefined-behaviour sanitizers, as a program of its own."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
// driver <command> <numbers ...>
//   beam     kind sharded small_fused beam_fused n max_particles beam_sort_min_particles profiling   -> 0 / 1
//   fused    kind sharded small_fused n max_particles palette_beams profiling                        -> 0 / 1 (batch_member_fused)
//   layout   members  n[members] B[members]              -> "blocks lds", then a line "first_beam" per member
//   search   members  first[members]  blocks ...         -> the member of every block
//   geometry                                             -> threads, particles per block, bytes per point, points at most
#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <vector>

#include "batch_host.h"

using namespace mcl;

static char** g_arg;
static unsigned long long uword() { return std::strtoull(*g_arg++, nullptr, 0); }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string_view what(argv[1]);
  g_arg = argv + 2;
  char** const end = argv + argc;
  if (what == "beam") {
    BatchBeamFacts m{};
    m.sensor_kind = static_cast<int>(uword());
    m.sharded = uword() != 0;
    m.small_fused = uword() != 0;
    m.beam_fused = uword() != 0;
    m.n = uword();
    m.max_particles = uword();
    m.beam_sort_min_particles = uword();
    m.profiling = uword() != 0;
    std::printf("%d\n", batch_beam_member_fused(m) ? 1 : 0);
  } else if (what == "fused") {
    BatchMemberFacts m{};
    m.sensor_kind = static_cast<int>(uword());
    m.sharded = uword() != 0;
    m.small_fused = uword() != 0;
    m.n = uword();
    m.max_particles = uword();
    m.palette_beams = uword() != 0;
    m.profiling = uword() != 0;
    std::printf("%d\n", batch_member_fused(m) ? 1 : 0);
  } else if (what == "layout") {
    const uint32_t members = static_cast<uint32_t>(uword());
    std::vector<uint64_t> n(members);
    std::vector<uint32_t> B(members), first(members);
    for (auto& v : n) v = uword();
    for (auto& v : B) v = static_cast<uint32_t>(uword());
    const BatchBeamGrid g = batch_beam_layout(n.data(), B.data(), members, first.data());
    std::printf("%u %u\n", g.blocks, g.lds);
    for (uint32_t m = 0; m < members; ++m) std::printf("%u %u\n", first[m], batch_beam_blocks(n[m], B[m]));
  } else if (what == "search") {
    const uint32_t members = static_cast<uint32_t>(uword());
    std::vector<uint32_t> first(members);
    for (auto& v : first) v = static_cast<uint32_t>(uword());
    while (g_arg < end) {
      const uint32_t block = static_cast<uint32_t>(uword());
      std::printf("%u\n", batch_member_of(members, block, [&](uint32_t m) { return first[m]; }));
    }
  } else if (what == "geometry") {
    std::printf("%u %u %u %u\n", kBatchBeamThreads, kBatchBeamBlock, kBatchBeamPointBytes, kBatchBeamMaxPoints);
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
                          ["-I", csrc, "-I", os.path.join(ROOT, "include"), str(src), os.path.join(csrc, "batch_host.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("batch_beam_host"), "driver", [])


def run(driver, what, *numbers):
    out = subprocess.check_output([driver, what] + [str(int(v)) for v in numbers], text=True)
    return [[int(w) for w in line.split()] for line in out.splitlines()]


# ---- which beam members ride on the fleet's launches ------------------------------------------------------------------------------------
LF, BEAM, LF_PROB, NDT, LANDMARK, BEARING = 0, 1, 2, 3, 4, 5
GOOD = dict(kind=BEAM, sharded=0, small_fused=1, beam_fused=1, n=2000, max_particles=2000, sort_min=16384, profiling=0)
BEAM_CASES = [
    (dict(), 1),
    (dict(kind=LF), 0), (dict(kind=LF_PROB), 0), (dict(kind=NDT), 0), (dict(kind=LANDMARK), 0), (dict(kind=BEARING), 0),
    (dict(sharded=1), 0),
    (dict(small_fused=0), 0),
    (dict(beam_fused=0), 0),
    (dict(n=0), 0), (dict(n=1), 1), (dict(n=4096, max_particles=4096), 1), (dict(n=4097, max_particles=4097), 0),
    (dict(n=300, max_particles=4096), 1), (dict(n=300, max_particles=4097), 0), (dict(max_particles=0), 0), (dict(max_particles=1), 1),
    (dict(sort_min=2001), 1), (dict(sort_min=2000), 0), (dict(sort_min=0), 0), (dict(n=1, sort_min=1), 0), (dict(n=1, sort_min=2), 1),
    (dict(profiling=1), 0),
]


def beam_fused(m):
    """Restated from the interface's paragraph: every condition has to hold."""
    return int(m["kind"] == BEAM and not m["sharded"] and bool(m["small_fused"]) and bool(m["beam_fused"]) and 1 <= m["n"] <= 4096 and
               1 <= m["max_particles"] <= 4096 and m["n"] < m["sort_min"] and not m["profiling"])


@pytest.mark.parametrize("change,want", BEAM_CASES)
def test_beam_eligibility_every_condition_flips_alone(driver, change, want):
    m = dict(GOOD, **change)
    assert beam_fused(m) == want
    got = run(driver, "beam", m["kind"], m["sharded"], m["small_fused"], m["beam_fused"], m["n"], m["max_particles"], m["sort_min"], m["profiling"])
    assert got == [[want]]


@pytest.mark.parametrize("n", [0, 1, 2000, 4096, 4097])
def test_the_likelihood_field_predicate_still_refuses_the_beam_kind(driver, n):
    assert run(driver, "fused", BEAM, 0, 1, n, max(n, 1), 1, 0) == [[0]]
    assert run(driver, "fused", BEAM, 0, 1, n, max(n, 1), 0, 0) == [[0]]


def test_geometry_restated(driver):
    """k_reweight_beam's: 256 threads, a wave of 64 per particle, a double2 per staged point, 64 KB at most."""
    assert run(driver, "geometry") == [[256, 256 // 64, 16, 64 * 1024 // 16]]


# ---- prefix, grid, the LDS maximum -----------------------------------------------------------------------------------------------------
def layout(n, B):
    """Restated: a running sum of ceil(n / 4) over the members with particles AND points; 16 bytes per point of the largest such scan."""
    first, blocks, total, lds = [], [], 0, 0
    for k, b in zip(n, B):
        first.append(total)
        own = -(-k // 4) if k and b else 0
        blocks.append(own)
        total += own
        if own:
            lds = max(lds, 16 * b)
    return [total, lds], list(zip(first, blocks))


FLEETS = {
    "edges_of_the_block": ([1, 4, 5, 4096], [180, 63, 4096, 1]),
    "empty_in_front_between_behind": ([0, 7, 0, 300, 9, 4096, 0, 33, 2000, 0], [180, 64, 0, 0, 65, 180, 4096, 0, 1, 0]),
    "one": ([777], [180]),
    "one_without_a_block": ([777], [0]),
    "thirty_three": ([61 + (i % 5) for i in range(33)], [16 + i for i in range(33)]),
    "thirty_three_with_gaps": ([0 if i % 4 == 1 else 1 + 3 * i for i in range(33)], [0 if i % 7 == 3 else 16 for i in range(33)]),
    "largest_scan_belongs_to_a_member_without_particles": ([0, 5, 9], [4096, 63, 64]),
    "none": ([], []),
}


@pytest.mark.parametrize("name", sorted(FLEETS))
def test_prefix_grid_and_lds_maximum(driver, name):
    n, B = FLEETS[name]
    out = run(driver, "layout", len(n), *n, *B)
    grid, firsts = layout(n, B)
    assert out[0] == grid
    assert [tuple(line) for line in out[1:]] == firsts


def test_layout_numbers_spelled_out(driver):
    n, B = FLEETS["edges_of_the_block"]
    out = run(driver, "layout", len(n), *n, *B)
    assert out[0] == [1 + 1 + 2 + 1024, 16 * 4096]
    assert [line[0] for line in out[1:]] == [0, 1, 2, 4]
    n, B = FLEETS["empty_in_front_between_behind"]
    out = run(driver, "layout", len(n), *n, *B)
    assert out[0] == [2 + 3 + 1024 + 500, 16 * 180]
    assert [line[0] for line in out[1:]] == [0, 0, 2, 2, 2, 5, 1029, 1029, 1029, 1529]


# ---- the block-to-member search over the beam prefix -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in sorted(FLEETS) if layout(*FLEETS[k])[0][0]])
def test_search_finds_the_member_of_every_block(driver, name):
    n, B = FLEETS[name]
    (total, _), firsts = layout(n, B)
    first = [f for f, _ in firsts]
    want = [m for m, (_, own) in enumerate(firsts) for _ in range(own)]
    assert len(want) == total
    got = run(driver, "search", len(n), *first, *range(total))
    assert [g[0] for g in got] == want


# ---- the same driver under the sanitizers, as a program of its own ---------------------------------------------------------------------------
def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = _compile(tmp_path, "driver_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    n, B = FLEETS["thirty_three_with_gaps"]
    (total, _), firsts = layout(n, B)
    for args in (["layout", len(n), *n, *B], ["layout", 0], ["layout", 1, 777, 0], ["search", len(n), *[f for f, _ in firsts], *range(total)],
                 ["search", 1, 0, 0, 5], ["beam", BEAM, 0, 1, 1, 2000, 2000, 16384, 0], ["fused", BEAM, 0, 1, 2000, 2000, 1, 0], ["geometry"]):
        done = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert done.returncode == 0 and "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr, (args, done.stderr)


# ---- header ----------------------------------------------------------------------------------------------------------------------------------
def test_header_names_the_option_and_the_counters():
    text = open(os.path.join(ROOT, "include", "beluga_mcl.h")).read()
    for word in ("batch_beam_fused", "beam_launches", "members_beam_fused"):
        assert re.search(r"\b" + word + r"\b", text), word
