"""The arithmetic of a batch of small filters (beluga_amd/csrc/batch_host.cpp) on the CPU, on the pattern of test_cycle_host_cpu.py: a
plain g++ compiles the file with a short driver that takes one command and its numbers and prints what the function returned.  Which
members share the launches, where their blocks lie, the block-to-member search as the kernels perform it, the workgroup memory of the
shared reweight and the validation of configs and scan offsets are checked against restatements written here, without a GPU; the same
driver runs once more under the address and undefined-behaviour sanitizers, as a program of its own."""
import ctypes as C
import os
import re
import subprocess

import pytest

from beluga_amd import build as mcl_build
from beluga_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
// driver <command> <numbers ...>
//   fused    kind sharded small_fused n max_particles palette_beams profiling   -> 0 / 1
//   layout   members  n[members] lds[members]                                   -> propagate_blocks reweight_blocks lds, then
//                                                                                  a line "first_propagate first_reweight" per member
//   search   members  first[members]  blocks ...                                -> the member of every block
//   offsets  members  offsets[members + 1]                                      -> 0 (fine) / 1
//   configs  count  (device stream)[count]     count = -1: null configs         -> 0 (fine) / 1
#include <cstdio>
#include <cstdlib>
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
  if (what == "fused") {
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
    std::vector<uint32_t> lds(members), fp(members), fr(members);
    for (auto& v : n) v = uword();
    for (auto& v : lds) v = static_cast<uint32_t>(uword());
    const BatchGrid g = batch_layout(n.data(), lds.data(), members, fp.data(), fr.data());
    std::printf("%u %u %u %u\n", g.members, g.propagate_blocks, g.reweight_blocks, g.reweight_lds);
    for (uint32_t m = 0; m < members; ++m) std::printf("%u %u\n", fp[m], fr[m]);
  } else if (what == "search") {
    const uint32_t members = static_cast<uint32_t>(uword());
    std::vector<uint32_t> first(members);
    for (auto& v : first) v = static_cast<uint32_t>(uword());
    while (g_arg < end) {
      const uint32_t block = static_cast<uint32_t>(uword());
      std::printf("%u\n", batch_member_of(members, block, [&](uint32_t m) { return first[m]; }));
    }
  } else if (what == "offsets") {
    const uint32_t members = static_cast<uint32_t>(uword());
    std::vector<uint64_t> offsets(members + 1);
    for (auto& v : offsets) v = uword();
    std::printf("%d\n", batch_check_offsets(offsets.data(), members) ? 1 : 0);
  } else if (what == "configs") {
    const long long count = std::strtoll(*g_arg++, nullptr, 0);
    if (count < 0) {
      std::printf("%d\n", batch_check_configs(nullptr, 1) ? 1 : 0);
      return 0;
    }
    std::vector<mcl_config> cfgs(static_cast<size_t>(count) + 1);
    for (long long i = 0; i < count && g_arg + 1 < end; ++i) {
      cfgs[i] = mcl_config{};
      cfgs[i].device_id = static_cast<int32_t>(uword());
      cfgs[i].hip_stream = reinterpret_cast<void*>(static_cast<uintptr_t>(uword()));
    }
    std::printf("%d\n", batch_check_configs(cfgs.data(), static_cast<uint32_t>(count)) ? 1 : 0);
  } else {
    return 2;
  }
  return 0;
}
"""


def _compile(tmp, name, extra):
    src = tmp / "driver.cpp"
    src.write_text("#include <string_view>\n" + DRIVER)
    exe = tmp / name
    csrc = os.path.join(ROOT, "beluga_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror"] + extra +
                          ["-I", csrc, "-I", os.path.join(ROOT, "include"), str(src), os.path.join(csrc, "batch_host.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("batch_host"), "driver", [])


def run(driver, what, *numbers):
    out = subprocess.check_output([driver, what] + [str(int(v)) for v in numbers], text=True)
    return [[int(w) for w in line.split()] for line in out.splitlines()]


# ---- which members share the launches ----------------------------------------------------------------------------------------------------
LF, BEAM, LF_PROB, NDT, LANDMARK, BEARING = 0, 1, 2, 3, 4, 5
GOOD = dict(kind=LF, sharded=0, small_fused=1, n=2000, max_particles=2000, palette_beams=1, profiling=0)
FUSED_CASES = [
    (dict(), 1),
    (dict(kind=LF_PROB), 1),
    (dict(kind=BEAM), 0), (dict(kind=NDT), 0), (dict(kind=LANDMARK), 0), (dict(kind=BEARING), 0),
    (dict(sharded=1), 0),
    (dict(small_fused=0), 0),
    (dict(n=4096, max_particles=4096), 1), (dict(n=4097, max_particles=4097), 0), (dict(n=0), 0), (dict(n=1), 1),
    (dict(n=300, max_particles=4097), 0), (dict(n=300, max_particles=4096), 1), (dict(max_particles=0), 0),
    (dict(palette_beams=0), 0),
    (dict(profiling=1), 0),
]


@pytest.mark.parametrize("change,want", FUSED_CASES)
def test_eligibility_every_condition_flips_alone(driver, change, want):
    m = dict(GOOD, **change)
    got = run(driver, "fused", m["kind"], m["sharded"], m["small_fused"], m["n"], m["max_particles"], m["palette_beams"], m["profiling"])
    assert got == [[want]]


# ---- prefixes, grids, the LDS maximum --------------------------------------------------------------------------------------------------
def layout(n, lds):
    """Restated: running sums of ceil(n / 256) and ceil(n / 4), the maximum of lds."""
    fp, fr, p, r = [], [], 0, 0
    for k in n:
        fp.append(p)
        fr.append(r)
        p += -(-k // 256)
        r += -(-k // 4)
    return [len(n), p, r, max(lds, default=0)], list(zip(fp, fr))


FLEETS = {
    "mixed": ([257, 301, 2000, 1234, 4096, 300], [392 + 8 * 40, 264 + 8 * 40, 392 + 8 * 41, 264 + 8 * 17, 392 + 8 * 40, 264 + 8 * 40]),
    "one": ([777], [1000]),
    "thirty_three": ([64] * 33, [500 + (i % 2) * 128 for i in range(33)]),
    "with_an_empty_member": ([1, 0, 256, 257, 0, 0, 4, 5], [8, 4096, 16, 8, 65536, 8, 8, 8]),
    "none": ([], []),
}


@pytest.mark.parametrize("name", sorted(FLEETS))
def test_prefixes_grids_and_lds_maximum(driver, name):
    n, lds = FLEETS[name]
    out = run(driver, "layout", len(n), *n, *lds)
    grid, firsts = layout(n, lds)
    assert out[0] == grid
    assert [tuple(line) for line in out[1:]] == firsts


def test_mixed_fleet_numbers(driver):
    """The fleet of the GPU test, spelled out: 2 + 2 + 8 + 5 + 16 + 2 propagation blocks, and the reweight's in fours."""
    n, lds = FLEETS["mixed"]
    out = run(driver, "layout", len(n), *n, *lds)
    assert out[0] == [6, 35, 65 + 76 + 500 + 309 + 1024 + 75, 392 + 8 * 41]
    assert [line[0] for line in out[1:]] == [0, 2, 4, 12, 17, 33]


# ---- the block-to-member search ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in sorted(FLEETS) if FLEETS[k][0]])
@pytest.mark.parametrize("per_block", [256, 4])
def test_search_at_every_first_and_last_block(driver, name, per_block):
    n, _ = FLEETS[name]
    blocks = [-(-k // per_block) for k in n]
    first = [sum(blocks[:m]) for m in range(len(n))]
    ask, want = [], []
    for m, (f, b) in enumerate(zip(first, blocks)):
        if b == 0:
            continue  # a member without a block is never found
        for block in sorted({f, f + b - 1, f + b // 2}):
            ask.append(block)
            want.append(m)
    got = run(driver, "search", len(n), *first, *ask)
    assert [g[0] for g in got] == want
    if len(ask) < sum(blocks) <= 4096:  # and every block there is
        every = run(driver, "search", len(n), *first, *range(sum(blocks)))
        assert [g[0] for g in every] == [m for m, b in enumerate(blocks) for _ in range(b)]


# ---- validation ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets,bad", [([0, 5, 5, 9], 0), ([3, 3, 3, 3], 0), ([0, 8, 4, 8], 1), ([9, 0, 0, 0], 1), ([0, 1, 2, 1], 1), ([0], 0)])
def test_point_offsets(driver, offsets, bad):
    assert run(driver, "offsets", len(offsets) - 1, *offsets) == [[bad]]


@pytest.mark.parametrize("cfgs,bad", [
    ([(0, 0)], 0), ([(0, 0), (0, 0), (0, 0)], 0), ([(2, 0x1000), (2, 0x1000)], 0),
    ([(0, 0), (1, 0)], 1), ([(0, 0), (0, 0x1000)], 1), ([(0, 0x1000), (0, 0)], 1), ([(0, 0x1000), (0, 0x2000)], 1),
    ([], 1), ([(0, 0)] * 1024, 0), ([(0, 0)] * 1025, 1),
])
def test_configs(driver, cfgs, bad):
    assert run(driver, "configs", len(cfgs), *[v for c in cfgs for v in c]) == [[bad]]


def test_null_configs(driver):
    out = subprocess.check_output([driver, "configs", "-1"], text=True)
    assert out.split() == ["1"]


# ---- the same driver under the sanitizers, as a program of its own ---------------------------------------------------------------------------
def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = _compile(tmp_path, "driver_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    n, lds = FLEETS["with_an_empty_member"]
    blocks = [-(-k // 4) for k in n]
    first = [sum(blocks[:m]) for m in range(len(n))]
    for args in (["layout", len(n), *n, *lds], ["layout", 0], ["search", len(n), *first, *range(sum(blocks))], ["search", 1, 0, 0, 5],
                 ["offsets", 3, 0, 8, 4, 8], ["offsets", 0, 7], ["configs", 3, 0, 0, 0, 0, 1, 0], ["configs", 0], ["configs", -1],
                 ["fused", 0, 0, 1, 2000, 2000, 1, 0]):
        done = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert done.returncode == 0 and "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr, (args, done.stderr)


# ---- header and bindings ----------------------------------------------------------------------------------------------------------------------
BATCH_SYMBOLS = ["mcl_batch_create", "mcl_batch_destroy", "mcl_batch_get_counter", "mcl_batch_last_error", "mcl_batch_member",
                 "mcl_batch_size", "mcl_batch_update"]


def test_header_declares_and_capi_binds_the_batch_entry_points():
    text = open(os.path.join(ROOT, "include", "beluga_mcl.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(mcl_[a-z0-9_]+)\s*\(", text)) if n.startswith("mcl_batch_"))
    assert declared == BATCH_SYMBOLS
    assert "typedef struct mcl_batch mcl_batch;" in text
    mcl_build.build()
    lib = capi.load()
    for name in BATCH_SYMBOLS:
        assert name in capi.exported_names()
        fn = getattr(lib, name)
        assert fn.argtypes is not None
    assert lib.mcl_batch_update.argtypes[-1] == C.POINTER(C.c_int32) and len(lib.mcl_batch_update.argtypes) == 7
    assert lib.mcl_batch_create.restype == C.c_int32 and lib.mcl_batch_last_error.restype == C.c_char_p
