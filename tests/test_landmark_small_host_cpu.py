"""The host decisions of the small landmark cycle (mcl_set_landmark_small_cycle) and of the fleet call mcl_landmark_batch_update on the
CPU, on the pattern of test_ndt_small_host_cpu.py: a plain g++ compiles batch_host.cpp and cycle_host.cpp with a short driver.  Which
lone cycle is the small one, which members ride on the fleet's launches, where their blocks lie in the shared reweight and which member
a block finds, and the offsets check.  In the same file, a restatement of the wave kernels' group search - the lane partition, the
per-lane strict scan, the xor reduction with the index tie rule - against the sequential first-of-equals pick."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
// driver <command> <numbers ...>
//   member    kind small_cycle sharded small_fused n max_particles profiling    -> 0 / 1 (batch_landmark_member_fused)
//   layout    members  n[members] k[members]         -> "blocks", then a line "first_landmark blocks" per member
//   search    members  first[members]  blocks ...    -> the member of every block
//   geometry                                         -> threads, particles per block, detections
//   small     small_cycle small_fused profiling n max_particles   -> 0 / 1 (landmark_cycle_is_small)
//   waves     small_cycle n                          -> 0 / 1 (landmark_reweight_takes_waves)
//   offsets   members offsets[members + 1]           -> 0 fine / 1 refused (batch_check_offsets); members 0 with no offsets: a null table
#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <vector>

#include "batch_host.h"
#include "cycle_host.h"

using namespace mcl;

static char** g_arg;
static unsigned long long uword() { return std::strtoull(*g_arg++, nullptr, 0); }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string_view what(argv[1]);
  g_arg = argv + 2;
  char** const end = argv + argc;
  if (what == "member") {
    BatchLandmarkFacts m{};
    m.sensor_kind = static_cast<int>(uword());
    m.small_cycle = uword() != 0;
    m.sharded = uword() != 0;
    m.small_fused = uword() != 0;
    m.n = uword();
    m.max_particles = uword();
    m.profiling = uword() != 0;
    std::printf("%d\n", batch_landmark_member_fused(m) ? 1 : 0);
  } else if (what == "layout") {
    const uint32_t members = static_cast<uint32_t>(uword());
    std::vector<uint64_t> n(members);
    std::vector<uint32_t> k(members), first(members);
    for (auto& v : n) v = uword();
    for (auto& v : k) v = static_cast<uint32_t>(uword());
    std::printf("%u\n", batch_landmark_layout(n.data(), k.data(), members, first.data()));
    for (uint32_t m = 0; m < members; ++m) std::printf("%u %u\n", first[m], batch_landmark_blocks(n[m], k[m]));
  } else if (what == "search") {
    const uint32_t members = static_cast<uint32_t>(uword());
    std::vector<uint32_t> first(members);
    for (auto& v : first) v = static_cast<uint32_t>(uword());
    while (g_arg < end) {
      const uint32_t block = static_cast<uint32_t>(uword());
      std::printf("%u\n", batch_member_of(members, block, [&](uint32_t m) { return first[m]; }));
    }
  } else if (what == "geometry") {
    std::printf("%u %u %u\n", kBatchLandmarkThreads, kBatchLandmarkBlock, kBatchLandmarkMaxDetections);
  } else if (what == "small") {
    LandmarkCycleFacts f{};
    f.small_cycle = uword() != 0;
    f.small_fused = uword() != 0;
    f.profiling = uword() != 0;
    f.n = uword();
    f.max_particles = uword();
    std::printf("%d\n", landmark_cycle_is_small(f) ? 1 : 0);
  } else if (what == "waves") {
    const bool on = uword() != 0;
    std::printf("%d\n", landmark_reweight_takes_waves(on, uword()) ? 1 : 0);
  } else if (what == "offsets") {
    const uint32_t members = static_cast<uint32_t>(uword());
    std::vector<uint64_t> off;
    while (g_arg < end) off.push_back(uword());
    std::printf("%d\n", batch_check_offsets(off.empty() ? nullptr : off.data(), members) ? 1 : 0);
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
    return _compile(tmp_path_factory.mktemp("landmark_small_host"), "driver", [])


def run_ints(driver, what, *numbers):
    out = subprocess.check_output([driver, what] + [str(int(v)) for v in numbers], text=True)
    return [[int(w) for w in line.split()] for line in out.splitlines()]


# ---- which lone cycle is the small one ------------------------------------------------------------------------------------------------
def small(driver, small_cycle=1, small_fused=1, profiling=0, n=2000, max_particles=2000):
    return run_ints(driver, "small", small_cycle, small_fused, profiling, n, max_particles)[0][0]


def test_size_rule_at_its_edges(driver):
    for n, want in [(0, 0), (1, 1), (4096, 1), (4097, 0)]:
        assert small(driver, n=n, max_particles=max(n, 1)) == want, n
        assert small(driver, n=min(max(n, 1), 4096), max_particles=n) == want, n  # (the bound has the same edges)
    assert small(driver, n=500, max_particles=4096) == 1 and small(driver, n=500, max_particles=4097) == 0


def test_size_rule_needs_the_switch_the_option_and_no_profiling(driver):
    assert small(driver) == 1
    assert small(driver, small_cycle=0) == 0
    assert small(driver, small_fused=0) == 0
    assert small(driver, profiling=1) == 0


def test_stage_level_reweight_takes_waves_up_to_4096(driver):
    for on, n, want in [(1, 0, 1), (1, 1, 1), (1, 4096, 1), (1, 4097, 0), (0, 1, 0), (0, 4096, 0)]:
        assert run_ints(driver, "waves", on, n)[0][0] == want, (on, n)


# ---- which members ride on the fleet's launches ----------------------------------------------------------------------------------------
LF, BEAM, LF_PROB, NDT, LANDMARK, BEARING = 0, 1, 2, 3, 4, 5
GOOD = dict(kind=LANDMARK, small_cycle=1, sharded=0, small_fused=1, n=2000, max_particles=2000, profiling=0)
MEMBER_CASES = [
    (dict(), 1), (dict(kind=BEARING), 1),
    (dict(kind=LF), 0), (dict(kind=BEAM), 0), (dict(kind=LF_PROB), 0), (dict(kind=NDT), 0),
    (dict(small_cycle=0), 0), (dict(sharded=1), 0), (dict(small_fused=0), 0), (dict(profiling=1), 0),
    (dict(n=0), 0), (dict(n=1, max_particles=1), 1), (dict(n=4096, max_particles=4096), 1), (dict(n=4097, max_particles=4097), 0),
    (dict(n=100, max_particles=0), 0), (dict(n=100, max_particles=4096), 1), (dict(n=100, max_particles=4097), 0),
]


def test_the_sensor_kinds_are_the_headers():
    text = open(os.path.join(ROOT, "include", "beluga_mcl.h")).read()
    for name, value in (("MCL_SENSOR_NDT", NDT), ("MCL_SENSOR_LANDMARK", LANDMARK), ("MCL_SENSOR_BEARING", BEARING)):
        assert re.search(name + r"\s*=\s*%d\b" % value, text), name


@pytest.mark.parametrize("change,want", MEMBER_CASES, ids=[",".join(f"{k}={v}" for k, v in c.items()) or "good" for c, _ in MEMBER_CASES])
def test_member_predicate(driver, change, want):
    m = dict(GOOD, **change)
    got = run_ints(driver, "member", m["kind"], m["small_cycle"], m["sharded"], m["small_fused"], m["n"], m["max_particles"], m["profiling"])
    assert got[0][0] == want


def test_member_predicate_is_the_lone_rule_for_an_unsharded_landmark_member(driver):
    for n in (0, 1, 4096, 4097):
        for bound in (0, 1, 4096, 4097):
            for switch, fused, prof in [(1, 1, 0), (0, 1, 0), (1, 0, 0), (1, 1, 1)]:
                lone = run_ints(driver, "small", switch, fused, prof, n, bound)[0][0]
                member = run_ints(driver, "member", LANDMARK, switch, 0, fused, n, bound, prof)[0][0]
                assert lone == member, (n, bound, switch, fused, prof)


# ---- where the members' blocks are -----------------------------------------------------------------------------------------------------
FLEETS = {
    "one": ([2000], [16]),
    "no_block_first_middle_last": ([0, 5, 7, 0, 4096, 1, 9], [3, 1, 0, 64, 64, 2, 0]),
    "none_has_a_block": ([0, 10, 0], [4, 0, 0]),
    "thirty_three": ([(i * 37) % 41 for i in range(33)], [(i * 5) % 3 for i in range(33)]),
}


def layout(n, k):
    blocks = [0 if (a == 0 or b == 0) else -(-a // 4) for a, b in zip(n, k)]
    return sum(blocks), [(sum(blocks[:m]), blocks[m]) for m in range(len(n))]


@pytest.mark.parametrize("name", sorted(FLEETS))
def test_layout_and_member_search(driver, name):
    n, k = FLEETS[name]
    out = run_ints(driver, "layout", len(n), *n, *k)
    total, firsts = layout(n, k)
    assert out[0] == [total] and [tuple(r) for r in out[1:]] == firsts
    if total:
        found = [r[0] for r in run_ints(driver, "search", len(n), *[f for f, _ in firsts], *range(total))]
        want = [m for m, (_, b) in enumerate(firsts) for _ in range(b)]
        assert found == want  # (a member without a block is never found)


def test_geometry_is_a_wave_per_particle_and_a_lane_per_detection(driver):
    assert run_ints(driver, "geometry") == [[256, 4, 64]]
    assert "#define MCL_LANDMARK_MAX_DETECTIONS 64" in open(os.path.join(ROOT, "include", "beluga_mcl.h")).read()


def test_offsets_check(driver):
    assert run_ints(driver, "offsets", 3, 0, 4, 4, 9)[0][0] == 0
    assert run_ints(driver, "offsets", 3, 5, 5, 5, 5)[0][0] == 0
    assert run_ints(driver, "offsets", 3, 0, 8, 4, 8)[0][0] == 1  # (decreasing)
    assert run_ints(driver, "offsets", 3)[0][0] == 1  # (a null table)


def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = _compile(tmp_path, "driver_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    n, k = FLEETS["no_block_first_middle_last"]
    total, firsts = layout(n, k)
    for args in (["layout", len(n), *n, *k], ["layout", 0], ["search", len(n), *[f for f, _ in firsts], *range(total)], ["search", 1, 0, 0, 5],
                 ["member", LANDMARK, 1, 0, 1, 2000, 2000, 0], ["small", 1, 1, 0, 4096, 4097], ["waves", 1, 4096], ["offsets", 3, 0, 8, 4, 8],
                 ["offsets", 2], ["geometry"]):
        done = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert done.returncode == 0 and "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr, (args, done.stderr)


# ---- the group search of the wave kernels, restated ---------------------------------------------------------------------------------------
NO_PICK = 0xFFFFFFFF


def group_of(k):
    """g = 64 / P with P the smallest power of two >= k."""
    P = 1
    while P < k:
        P *= 2
    return 64 // P


def beats(larger, v, at, other_v, other_at):
    if other_at == NO_PICK:
        return True
    if at == NO_PICK:
        return False
    if v == other_v:
        return at < other_at
    return v > other_v if larger else v < other_v


def wave_picks(values_per_record, larger):
    """The 64 lanes of a wave over k records: record j owns lanes [j g, (j + 1) g); lane r scans r, r + g, ... in ascending order and
    replaces on a strictly better value; log2 g xor steps over the WHOLE wave's lanes (they stay inside the aligned groups).  Returns the
    pick that the first lane of every record's group holds, and checks that every lane of the group agrees."""
    k = len(values_per_record)
    g = group_of(k)
    value, at = [0.0] * 64, [NO_PICK] * 64
    for lane in range(64):
        j, r = lane // g, lane % g
        if j >= k:
            continue
        v = values_per_record[j]
        for t in range(r, len(v), g):
            if t == r or (v[t] > value[lane] if larger else v[t] < value[lane]):
                value[lane], at[lane] = v[t], t
    step = g // 2
    while step >= 1:
        nv, na = list(value), list(at)
        for lane in range(64):
            other = lane ^ step
            assert other // g == lane // g  # (the xor step stays inside the aligned group)
            if not beats(larger, value[lane], at[lane], value[other], at[other]):
                nv[lane], na[lane] = value[other], at[other]
        value, at = nv, na
        step //= 2
    for j in range(k):
        assert len(set(at[j * g:(j + 1) * g])) == 1
    return [at[j * g] for j in range(k)]


def sequential_pick(v, larger):
    """std::min_element / the lane kernel's scan: the first of equal ones."""
    if len(v) == 0:
        return NO_PICK
    best = 0
    for t in range(1, len(v)):
        if (v[t] > v[best]) if larger else (v[t] < v[best]):
            best = t
    return best


def test_group_sizes():
    assert [group_of(k) for k in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)] == [64, 32, 16, 16, 8, 8, 4, 4, 2, 2, 1, 1]
    for k in range(1, 65):
        g = group_of(k)
        P = 64 // g
        assert P >= k and (P == 1 or P // 2 < k) and P & (P - 1) == 0  # (the smallest power of two >= k)


@pytest.mark.parametrize("larger", [False, True], ids=["min", "max"])
def test_group_search_is_the_sequential_first_of_equals(larger):
    rng = np.random.Generator(np.random.PCG64(5))
    for k in range(1, 65):
        g = group_of(k)
        lengths = sorted({L for L in (0, 1, 2, g - 1, g, g + 1, 65, 130) if L >= 0})
        for L in lengths:
            # distinct values; then coarse values with many equal ones
            for values in (rng.permutation(L * k).reshape(k, L).astype(float), rng.integers(0, 3, (k, L)).astype(float)):
                records = [list(row) for row in values]
                assert wave_picks(records, larger) == [sequential_pick(v, larger) for v in records], (k, L)


@pytest.mark.parametrize("larger", [False, True], ids=["min", "max"])
def test_group_search_with_planted_ties(larger):
    best = 9.0 if larger else -9.0
    for k in range(1, 65):
        g = group_of(k)
        L = 130
        # index pairs in the same lane (a, a + g), (a, a + 2g) and in different lanes
        pairs = {(0, g), (1, 1 + 2 * g), (g - 1, 2 * g - 1), (0, 1), (0, g - 1), (1, g), (g - 1, g), (5, 129), (64, 65), (3, 3 + g + 1)}
        for a, b in sorted(p for p in pairs if p[0] < p[1] < L):
            v = [float(t % 7) for t in range(L)]
            v[a] = v[b] = best
            records = [list(v) for _ in range(k)]
            assert wave_picks(records, larger) == [a] * k, (k, a, b)
            if g > 1:
                assert (a % g == b % g) == ((b - a) % g == 0)


def test_a_lane_that_scanned_nothing_loses_even_to_the_worst_value():
    for larger in (False, True):
        worst = -math.inf if larger else math.inf
        for k in (1, 2, 8):
            assert wave_picks([[worst]] * k, larger) == [0] * k
            assert wave_picks([[worst, worst, worst]] * k, larger) == [0] * k
            assert wave_picks([[]] * k, larger) == [NO_PICK] * k


# ---- header and bindings ---------------------------------------------------------------------------------------------------------------------
def test_header_and_bindings_name_the_calls():
    import ctypes as C

    from beluga_amd import capi
    text = open(os.path.join(ROOT, "include", "beluga_mcl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for word in ("mcl_set_landmark_small_cycle", "mcl_get_landmark_small_cycle", "mcl_landmark_batch_update"):
        assert re.search(r"\b" + word + r"\s*\(", code), word
        assert word in capi.exported_names() and word in capi._OPTIONAL
    for word in ("landmark_wave_launches", "landmark_launches", "members_landmark_fused"):
        assert word in text
    # the prototypes against the header's parameter lists
    def params(name):
        return [p.strip() for p in re.search(r"\b" + name + r"\s*\(([^)]*)\)", code).group(1).split(",")]
    assert params("mcl_set_landmark_small_cycle") == ["mcl_ctx* ctx", "int32_t on"]
    assert params("mcl_get_landmark_small_cycle") == ["mcl_ctx* ctx", "int32_t* on"]
    assert params("mcl_landmark_batch_update") == ["mcl_batch* batch", "const double* control_poses", "const double* vectors_xyz",
                                                   "const uint32_t* categories", "const uint64_t* detection_offsets", "mcl_estimate* estimates",
                                                   "mcl_update_info* infos", "mcl_status* statuses"]
    sig = capi._SIGNATURES
    assert sig["mcl_set_landmark_small_cycle"] == (C.c_int32, [capi._ctx, C.c_int32])
    assert sig["mcl_get_landmark_small_cycle"] == (C.c_int32, [capi._ctx, C.POINTER(C.c_int32)])
    assert sig["mcl_landmark_batch_update"] == (C.c_int32, [capi._batch, capi.c_double_p, capi.c_double_p, capi.c_u32_p, capi.c_u64_p,
                                                            C.POINTER(capi.Estimate), C.POINTER(capi.UpdateInfo), C.POINTER(C.c_int32)])
