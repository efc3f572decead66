"""What a shared map decides without a device (beluga_amd/csrc/map_store_host.{h,cpp}), on the pattern of test_batch_cpu.py: a plain g++
compiles the file with a short driver that takes one command and its numbers and prints what the function returned.  Which contexts may
read a store, the bytes a store holds against sums written out by hand, and a context's counted hold on a store (MapHold) with a store
type that owns heap memory instead of device memory; the same driver runs once more under the address and undefined-behaviour
sanitizers, as a program of its own.  And the header, capi.py and the library agree on the five entry points."""
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
//   kind      sensor_kind                                                    -> 0 (fine) / 1
//   mismatch  store_device store_kind  ctx_device ctx_kind  field delta      -> "ok" or the reason; the context's mcl_lf_params are the
//                                                                               store's with field `field` (0 .. 6, 7: none) off by delta
//   layout    W H                                                            -> tiles_x tiles_y pal_base palette_possible max_entries
//                                                                               pal_idx_count pal_pitch pal_bytes far_row_bytes far_bytes
//                                                                               far_possible far_linear_bytes
//   bytes     kind W H n_free nonfree_words pal_count far_tiles              -> device host
//   hold      contexts                                                       -> a script of attaches, swaps and releases; prints the
//                                                                               users and the live stores after every step
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string_view>
#include <vector>

#include "map_store_host.h"

using namespace mcl;

static char** g_arg;
static long long word() { return std::strtoll(*g_arg++, nullptr, 0); }

// A store that owns heap memory the way MapStore owns device memory: read through the hold, freed with the last reference.
static int g_live = 0;
struct FakeStore {
  mutable std::atomic<uint32_t> users{0};
  int* cells{nullptr};
  int value{0};
  explicit FakeStore(int v) : cells(new int[64]), value(v) {
    for (int i = 0; i < 64; ++i) cells[i] = v;
    ++g_live;
  }
  FakeStore() = default;
  FakeStore(const FakeStore&) = delete;
  ~FakeStore() {
    if (cells) --g_live;
    delete[] cells;
  }
};
static int peek(const MapHold<FakeStore>& h) { return h->cells ? h->cells[63] : -1; }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string_view what(argv[1]);
  g_arg = argv + 2;
  if (what == "kind") {
    std::printf("%d\n", map_store_check_kind(static_cast<int32_t>(word())) ? 1 : 0);
  } else if (what == "mismatch") {
    const mcl_lf_params lf{2.0, 100.0, 0.5, 0.5, 0.2, 1, 0};
    MapStoreKey key{static_cast<int32_t>(word()), 0, lf};
    key.sensor_kind = static_cast<int32_t>(word());
    const int32_t device = static_cast<int32_t>(word()), kind = static_cast<int32_t>(word());
    const long long field = word();
    const double delta = std::strtod(*g_arg++, nullptr);
    mcl_lf_params mine = lf;
    double* doubles[5] = {&mine.max_obstacle_distance, &mine.max_laser_distance, &mine.z_hit, &mine.z_random, &mine.sigma_hit};
    if (field >= 0 && field < 5) *doubles[field] += delta;
    if (field == 5) mine.model_unknown_space = 0;
    if (field == 6) mine.only_obstacle_boundaries = 1;
    const char* why = map_store_mismatch(key, device, kind, mine);
    std::printf("%s\n", why ? why : "ok");
  } else if (what == "layout") {
    const uint32_t W = static_cast<uint32_t>(word()), H = static_cast<uint32_t>(word());
    const MapTableLayout t = map_table_layout(W, H);
    std::printf("%llu %llu %u %d %u %llu %u %u %u %u %d %u\n", (unsigned long long)t.tiles_x, (unsigned long long)t.tiles_y, t.pal_base,
                t.palette_possible ? 1 : 0, t.max_entries, (unsigned long long)t.pal_idx_count, t.pal_pitch, t.pal_bytes, t.far_row_bytes,
                t.far_bytes, t.far_possible ? 1 : 0, t.far_linear_bytes);
  } else if (what == "bytes") {
    MapStoreShape s{};
    s.sensor_kind = static_cast<int32_t>(word());
    s.W = static_cast<uint32_t>(word());
    s.H = static_cast<uint32_t>(word());
    s.n_free = static_cast<uint64_t>(word());
    s.nonfree_words = static_cast<uint64_t>(word());
    s.pal_count = static_cast<uint32_t>(word());
    s.far_tiles = word() != 0;
    const MapStoreBytes b = map_store_bytes(s);
    std::printf("%llu %llu\n", (unsigned long long)b.device, (unsigned long long)b.host);
  } else if (what == "hold") {
    const int contexts = static_cast<int>(word());
    auto say = [&](const char* step, const std::shared_ptr<const FakeStore>& a, const std::shared_ptr<const FakeStore>& b) {
      std::printf("%s %d %d %d\n", step, a ? static_cast<int>(a->users.load()) : -1, b ? static_cast<int>(b->users.load()) : -1, g_live);
    };
    {
      std::vector<std::unique_ptr<MapHold<FakeStore>>> holds;
      for (int i = 0; i < contexts; ++i) holds.push_back(std::make_unique<MapHold<FakeStore>>(std::make_shared<FakeStore>()));
      std::shared_ptr<const FakeStore> a = std::make_shared<FakeStore>(7), b = std::make_shared<FakeStore>(9);
      say("built", a, b);
      for (auto& h : holds) h->attach(a);
      say("attached", a, b);
      holds[0]->attach(a);  // the store it holds already
      say("again", a, b);
      const FakeStore* raw_a = a.get();
      a.reset();            // the caller's reference goes; the contexts still read
      int sum = 0;
      for (auto& h : holds) sum += peek(*h);
      std::printf("read %d %u %d\n", sum, raw_a->users.load(), g_live);
      holds[0]->attach(b);  // a swap
      say("swapped", holds[1]->ptr(), b);
      holds[1]->own(std::make_shared<FakeStore>(3));  // mcl_set_map on an attached context: a private store, not counted
      std::printf("private %d %d %d %d\n", peek(*holds[1]), holds[1]->shared() ? 1 : 0, static_cast<int>(holds[1]->ptr()->users.load()), g_live);
      std::printf("take_shared %d\n", holds[0]->take_private() ? 1 : 0);
      {
        const std::shared_ptr<FakeStore> old = holds[1]->take_private();
        std::printf("take_private %d %d %d\n", old ? old->cells[0] : -1, peek(*holds[1]), g_live);
      }
      std::printf("taken %d\n", g_live);
      for (size_t i = 2; i < holds.size(); ++i) holds[i]->drop();  // the last readers of a leave: it dies here
      std::printf("dropped %d %d\n", static_cast<int>(b->users.load()), g_live);
      b.reset();
      std::printf("b_released %d %d\n", peek(*holds[0]), g_live);
    }
    std::printf("end %d\n", g_live);
  } else {
    return 2;
  }
  return 0;
}
"""


def compile_driver(tmp, name, extra=()):
    src = tmp / "driver.cpp"
    src.write_text(DRIVER)
    exe = tmp / name
    csrc = os.path.join(ROOT, "beluga_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror"] + list(extra) +
                          ["-I", csrc, "-I", os.path.join(ROOT, "include"), str(src), os.path.join(csrc, "map_store_host.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("map_store_host"), "driver")


def run(driver, what, *numbers):
    return subprocess.check_output([driver, what] + [str(v) for v in numbers], text=True).splitlines()


def store_bytes(driver, kind, W, H, n_free, nonfree_words, pal_count, far_tiles):
    """(device, host) bytes of a store built from nothing (also what test_gpu_shared_map.py holds mcl_shared_map_info to)."""
    return tuple(int(v) for v in run(driver, "bytes", kind, W, H, n_free, nonfree_words, pal_count, int(far_tiles))[0].split())


LF, BEAM, LF_PROB, NDT, LANDMARK, BEARING = 0, 1, 2, 3, 4, 5


# ---- who may read a store ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,bad", [(LF, 0), (BEAM, 0), (LF_PROB, 0), (NDT, 1), (LANDMARK, 1), (BEARING, 1), (-1, 1), (6, 1)])
def test_kinds_with_an_occupancy_grid(driver, kind, bad):
    assert run(driver, "kind", kind) == [str(bad)]


LF_FIELDS = ["max_obstacle_distance", "max_laser_distance", "z_hit", "z_random", "sigma_hit", "model_unknown_space", "only_obstacle_boundaries"]


@pytest.mark.parametrize("kind", [LF, LF_PROB])
def test_equal_configs_are_accepted(driver, kind):
    assert run(driver, "mismatch", 0, kind, 0, kind, 7, 0) == ["ok"]
    assert run(driver, "mismatch", 3, kind, 3, kind, 7, 0) == ["ok"]


@pytest.mark.parametrize("kind", [LF, LF_PROB])
def test_every_single_field_difference_is_refused_with_its_own_reason(driver, kind):
    reasons = []
    for field, name in enumerate(LF_FIELDS):
        for delta in (1e-12, -0.125):  # (the smallest difference counts: the tables are functions of the exact values)
            (why,) = run(driver, "mismatch", 0, kind, 0, kind, field, delta)
            assert why.startswith("mcl_use_shared_map: ") and ("lf." + name) in why, why
            assert [n for n in LF_FIELDS if ("lf." + n + " ") in why] == [name], why
        reasons.append(why)
    assert len(set(reasons)) == len(LF_FIELDS)


def test_kind_family_and_device_are_refused(driver):
    (lf_prob,) = run(driver, "mismatch", 0, LF, 0, LF_PROB, 7, 0)
    (prob_lf,) = run(driver, "mismatch", 0, LF_PROB, 0, LF, 7, 0)
    assert "sensor_kind" in lf_prob and lf_prob == prob_lf
    (beam_on_lf,) = run(driver, "mismatch", 0, LF, 0, BEAM, 7, 0)
    (lf_on_beam,) = run(driver, "mismatch", 0, BEAM, 0, LF, 7, 0)
    (prob_on_beam,) = run(driver, "mismatch", 0, BEAM, 0, LF_PROB, 7, 0)
    assert "beam" in beam_on_lf and beam_on_lf == lf_on_beam == prob_on_beam and beam_on_lf != lf_prob
    for kind in (LF, BEAM, LF_PROB):
        (device,) = run(driver, "mismatch", 0, kind, 1, kind, 7, 0)
        assert "device" in device and device not in (lf_prob, beam_on_lf)


def test_beam_contexts_do_not_compare_likelihood_field_parameters(driver):
    for field in range(7):
        assert run(driver, "mismatch", 0, BEAM, 0, BEAM, field, 0.5) == ["ok"]


# ---- bytes ---------------------------------------------------------------------------------------------------------------------------------
def test_table_layout_of_a_size_off_the_tile(driver):
    """101 x 75 cells: 13 x 10 tiles of 8 x 8 and a border tile on every side = 15 x 12; the row-offset table of 77 rows, 4 bytes each,
    rounded up to 8 = 312 bytes; 2 bytes per cell of every tile; the far bitmap in rows of ceil(15 / 8) = 2 bytes, 24 -> 32 bytes."""
    assert run(driver, "layout", 101, 75) == ["15 12 312 1 2048 11520 1920 23040 2 32 1 32"]
    # exactly on the tile: no extra tile
    assert run(driver, "layout", 96, 64)[0].split()[:2] == ["14", "10"]
    assert run(driver, "layout", 97, 65)[0].split()[:2] == ["15", "11"]
    # a table beyond what 32 bits of byte offset address: no palette
    assert run(driver, "layout", 40000, 40000)[0].split()[3] == "0"


BYTES_CASES = [
    # likelihood field, 101 x 75 = 7575 cells, 5000 free, 300 palette entries, far tiles: occupancy 7575 + free list 20000 + field 30300
    # + pz^3 table 8 * 7576 = 60608 + keys and values 12 * 300 = 3600 + index 2 * 11520 = 23040 + votes 1200 + far 32 + linear 32
    ((LF, 101, 75, 5000, 0, 300, 1), (7575 + 20000 + 30300 + 60608 + 3600 + 23040 + 1200 + 32 + 32, 30300)),
    # the same without a far-tile winner: the bitmap by rows was allocated for the vote, the linear one was not
    ((LF_PROB, 101, 75, 5000, 0, 300, 0), (7575 + 20000 + 30300 + 60608 + 3600 + 23040 + 1200 + 32, 30300)),
    # no palette (too many distinct values): occupancy, free list, field, pz^3 table
    ((LF, 101, 75, 5000, 0, 0, 0), (7575 + 20000 + 30300 + 60608, 30300)),
    # no free cell: the list keeps one slot.  128 x 64 = 8192 cells, 18 x 10 tiles
    ((LF, 128, 64, 0, 0, 2, 0), (8192 + 4 + 32768 + 65544 + 24 + 2 * 18 * 10 * 64 + 8 + 32, 32768)),
    # beam model: occupancy, free list, packed occupancy; no field on either side
    ((BEAM, 101, 75, 5000, 777, 0, 0), (7575 + 20000 + 4 * 777, 0)),
    # 1 x 1
    ((LF, 1, 1, 1, 0, 1, 1), (1 + 4 + 4 + 16 + 12 + 2 * 9 * 64 + 4 + 16 + 16, 4)),
]


@pytest.mark.parametrize("shape,want", BYTES_CASES)
def test_bytes_against_hand_sums(driver, shape, want):
    assert store_bytes(driver, *shape) == want


def test_headline_map_bytes_per_cell(driver):
    """DESIGN.md's table: 15 B per cell plus 4 B per free cell on the device, 4 B per cell on the host, at 4000 x 4000."""
    cells = 4000 * 4000
    device, host = store_bytes(driver, LF, 4000, 4000, cells // 2, 0, 400, 1)
    assert host == 4 * cells
    assert 15.0 <= (device - 4 * (cells // 2)) / cells < 15.1


# ---- a context's hold on a store -------------------------------------------------------------------------------------------------------------
HOLD_SCRIPT = [
    "built 0 0 2",          # two stores, nobody attached
    "attached 4 0 2",
    "again 4 0 2",          # attaching the store already held counts once
    "read 28 4 2",          # the caller's reference is gone: four contexts still read 7 each
    "swapped 3 1 2",        # one context moved to b
    "private 3 0 0 3",      # a private store: read, not shared, not counted; a lost a user below
    "take_shared 0",        # a shared hold gives nothing up
    "take_private 3 -1 3",  # a private one gives its store up and holds no map
    "taken 2",              # ... and the store died with its taker
    "dropped 1 1",          # the last two readers of a left: a died, b lives
    "b_released 9 1",       # b without its caller's reference: the context that reads it keeps it alive
    "end 0",
]


def test_hold_counts_users_and_keeps_stores_alive(driver):
    assert run(driver, "hold", 4) == HOLD_SCRIPT


# ---- the same driver under the sanitizers, as a program of its own -------------------------------------------------------------------------------
def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = compile_driver(tmp_path, "driver_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for args in (["hold", 4], ["hold", 9], ["layout", 101, 75], ["layout", 1, 1], ["layout", 40000, 40000], ["layout", 65535, 65535],
                 ["bytes", LF, 101, 75, 5000, 0, 300, 1], ["bytes", BEAM, 1, 1, 0, 3, 0, 0], ["bytes", LF, 65535, 65535, 0, 0, 9, 1],
                 ["mismatch", 0, LF, 0, LF, 7, 0], ["mismatch", 0, LF, 0, LF, 4, 0.5], ["mismatch", 0, BEAM, 1, LF_PROB, 7, 0], ["kind", NDT]):
        done = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert done.returncode == 0 and "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr, (args, done.stderr)
        if args[0] == "hold":
            assert done.stdout.splitlines()[-1] == "end 0"


# ---- header and bindings ---------------------------------------------------------------------------------------------------------------------
SHARED_MAP_SYMBOLS = ["mcl_shared_map_create", "mcl_shared_map_get_info", "mcl_shared_map_last_error", "mcl_shared_map_release",
                      "mcl_use_shared_map"]


def test_header_declares_and_capi_binds_the_shared_map_entry_points(tmp_path):
    text = open(os.path.join(ROOT, "include", "beluga_mcl.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(mcl_[a-z0-9_]+)\s*\(", text)) if "shared_map" in n)
    assert declared == SHARED_MAP_SYMBOLS
    assert "typedef struct mcl_shared_map mcl_shared_map;" in text
    mcl_build.build()
    lib = capi.load()
    for name in SHARED_MAP_SYMBOLS:
        assert name in capi.exported_names()
        assert getattr(lib, name).argtypes is not None
    assert len(lib.mcl_shared_map_create.argtypes) == 9 and lib.mcl_shared_map_create.restype == C.c_int32
    assert lib.mcl_shared_map_release.restype is None and lib.mcl_shared_map_last_error.restype == C.c_char_p
    assert len(lib.mcl_use_shared_map.argtypes) == 2
    # the info struct as a C compiler lays it out
    src = tmp_path / "info.c"
    src.write_text('#include <stdio.h>\n#include "beluga_mcl.h"\nint main(void){printf("%zu %zu %zu\\n", sizeof(mcl_shared_map_info), '
                   'offsetof(mcl_shared_map_info, device_bytes), offsetof(mcl_shared_map_info, users));return 0;}')
    exe = tmp_path / "info"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out == [C.sizeof(capi.SharedMapInfo), capi.SharedMapInfo.device_bytes.offset, capi.SharedMapInfo.users.offset]


def test_refusals_that_need_no_device():
    """Null arguments and the kinds without an occupancy grid are refused before any device is looked for."""
    mcl_build.build()
    lib = capi.load()
    cfg = capi.Config()
    lib.mcl_default_config(C.byref(cfg))
    handle = capi._shared_map()
    cells = (C.c_int8 * 4)(0, 0, 100, 0)
    origin = (C.c_double * 4)(1.0, 0.0, 0.0, 0.0)
    traits = (C.c_int8 * 3)(0, -1, 100)
    for kind in (capi.MCL_SENSOR_NDT, capi.MCL_SENSOR_LANDMARK, capi.MCL_SENSOR_BEARING):
        cfg.sensor_kind = kind
        assert lib.mcl_shared_map_create(C.byref(cfg), cells, 2, 2, 0.05, origin, traits, 0, C.byref(handle)) == capi.MCL_ERR_UNSUPPORTED
        assert not handle.value and b"occupancy-grid" in lib.mcl_shared_map_last_error(None)
    cfg.sensor_kind = capi.MCL_SENSOR_LIKELIHOOD_FIELD
    assert lib.mcl_shared_map_create(C.byref(cfg), None, 2, 2, 0.05, origin, traits, 0, C.byref(handle)) == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.mcl_shared_map_create(C.byref(cfg), cells, 2, 2, 0.05, origin, traits, 2, C.byref(handle)) == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.mcl_shared_map_create(None, cells, 2, 2, 0.05, origin, traits, 0, C.byref(handle)) == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.mcl_shared_map_get_info(None, None) == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.mcl_use_shared_map(None, None) == capi.MCL_ERR_INVALID_ARGUMENT
    lib.mcl_shared_map_release(None)  # (as free(NULL))
