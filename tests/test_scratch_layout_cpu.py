"""The layouts of the carved scratch buffers (beluga_amd/csrc/scratch_layout.h) on the CPU: a plain g++ compiles the header with a short
driver that prints, for each layout and each set of parameters, every area's byte offset, byte length and alignment and every buffer's
size.  The assertions: the areas of a buffer are disjoint and end inside it; the size is no smaller than the expression the buffer was
sized by before the header existed; every area lies at the offset it had then; every area is aligned to its element.

parent() below is that earlier arithmetic, written out literally from context.hip's ensure() arguments and pointer sums and from the
launchers of kernels.hip (`sort->totals + kSortDigits`, `sort->bbox + 8`) as they stood before this header: it is what pins "no area
moves", and it is never derived from the header.

Alignment.  An area's element is its scalar type, except the cell list's states: double4 records, which want 16 bytes.  They lie
`capacity` doubles behind the head of the list's f64 area, so a list's capacity must be a multiple of 4 (cell_list_capacity).  For a
list in ONE block (the mapped host list, the host's copy of a large list) the callers always rounded up to one, and the block cases
here are the grid's capacities rounded up likewise.  The DEVICE arrays hold a list for as many cells as the context has particles,
any number, and before this header they were laid out for that number itself: the states lay (table_capacity + capacity) doubles
into d_cell_f64, 8 bytes off a 16-byte boundary for every odd capacity (of the grid: 1, 255, 257, 1023, 1025, 262143, 262145).  No
layout has both those offsets and aligned states, so ClusterLayout lays the device list out for cell_list_capacity(capacity).  THE ONE
PLACE WHERE AN AREA MOVES: with a particle capacity that is no multiple of 4, the device list's areas behind the first of each type
(state; count, slot, cluster, size) lie up to 3 elements per array before them further back than they did, in buffers that much larger;
with a multiple of 4 nothing moves.  parent() says so in its cluster rows: the earlier expressions, literally, over the list's capacity
- which was the particle capacity and is that rounded up to 4 - while the sizes are held to the earlier ensure() arguments at the
particle capacity itself; test_the_device_list_moves_only_for_capacities_that_are_no_multiple_of_4 pins the exception down."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
// driver kind:a,b ...   One line per argument: <argument>|<buffer>.<area>,<byte offset>,<byte length>,<alignment>|...|=<buffer>,<bytes>|...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "scratch_layout.h"

using namespace mcl;

namespace {
void area(const char* name, size_t offset, size_t count, size_t element, size_t alignment = 0) {
  std::printf("|%s,%zu,%zu,%zu", name, offset * element, count * element, alignment ? alignment : element);
}
void total(const char* buffer, size_t count, size_t element) { std::printf("|=%s,%zu", buffer, count * element); }
void rows(const char* buffer, const RowsLayout& r, size_t element) {
  for (size_t k = 0; k < r.rows; ++k) area((std::string(buffer) + ".row" + std::to_string(k)).c_str(), r.row(k), r.stride, element);
  total(buffer, r.size(), element);
}
// a cell list's areas, `at_*` elements into the buffers of its three types
void cell_list(const CellListLayout& l, const char* u64, size_t at_u64, const char* f64, size_t at_f64, const char* u32, size_t at_u32) {
  const size_t c = l.capacity;
  area((std::string(u64) + ".key").c_str(), at_u64 + l.key, c, 8);
  area((std::string(f64) + ".wsum").c_str(), at_f64 + l.wsum, c, 8);
  area((std::string(f64) + ".state").c_str(), at_f64 + l.state, 4 * c, 8, 16);
  area((std::string(u32) + ".first").c_str(), at_u32 + l.first, c, 4);
  area((std::string(u32) + ".count").c_str(), at_u32 + l.count, c, 4);
  area((std::string(u32) + ".slot").c_str(), at_u32 + l.slot, c, 4);
  area((std::string(u32) + ".cluster").c_str(), at_u32 + l.cluster, c, 4);
  area((std::string(u32) + ".size").c_str(), at_u32 + l.size_word, 1, 4);
}
}  // namespace

int main(int argc, char** argv) {
  for (int k = 1; k < argc; ++k) {
    std::string name(argv[k]);
    unsigned long long a[3] = {0, 0, 0};
    if (const size_t colon = name.find(':'); colon != std::string::npos) {
      const char* p = argv[k] + colon + 1;
      for (int j = 0; j < 3 && *p; ++j) {
        char* end = nullptr;
        a[j] = std::strtoull(p, &end, 10);
        p = *end ? end + 1 : end;
      }
      name.resize(colon);
    }
    std::printf("%s", argv[k]);
    if (name == "sort") {
      const SortLayout l(a[0]);
      area("u32.keys", l.keys, a[0], 4);
      area("u32.perm", l.perm, a[0], 4);
      area("u32.table", l.table, kSortDigits * l.nblocks, 4);
      area("u32.totals", l.totals, kSortDigits, 4);
      area("u32.bases", l.bases, kSortDigits, 4);
      area("u32.flags", l.flags, kSortFlagWords, 4);
      total("u32", l.u32_size, 4);
      area("u64.keyidx", l.keyidx, a[0], 8);
      total("u64", l.u64_size, 8);
      area("f64.frame", l.frame, kKeyFrameDoubles, 8);
      area("f64.bbox", l.bbox, 8, 8);
      area("f64.bbox_partials", l.bbox_partials, 6 * l.nblocks, 8);
      area("f64.partial", l.partial, kLfMaxSegments * std::min<uint64_t>(a[0], kLfSegmentedBelow), 8);
      area("f64.spare_row", l.spare_row, 6, 8);
      total("f64", l.f64_size, 8);
    } else if (name == "chunk") rows("chunk", chunk_rows(a[0]), 8);
    else if (name == "kld") rows("uchunk", kld_chunk_rows(a[0]), 4);
    else if (name == "est") rows("est", estimate_rows(a[0]), 8);
    else if (name == "draw") rows("partials", draw_estimate_rows(a[0]), 8);
    else if (name == "xchg") rows("exchange", cell_exchange_rows(7, a[0], static_cast<uint32_t>(a[1])), 8);
    else if (name == "ndtw") rows("words", ndt_word_rows(static_cast<uint32_t>(a[0])), 8);
    else if (name == "lfw") total("wsum", lf_weight_sums_size(a[0]), 8);
    else if (name == "route") {
      const RouteLayout l(static_cast<uint32_t>(a[0]), a[1]);
      area("u32.block_hist", l.block_hist, l.hist, 4);
      area("u32.chunk_sum", l.chunk_sum, l.hist / kChunk + 1, 4);
      area("u32.chunk_off", l.chunk_off, l.hist / kChunk + 1, 4);
      std::printf("|u32.dest,%zu,%llu,1", l.dest * 4, a[1]);  // one byte per target
      area("u32.slack", l.slack, kRouteSlackWords, 4);
      total("u32", l.size, 4);
    } else if (name == "ndt") {
      const uint32_t n = static_cast<uint32_t>(a[0]);
      const NdtBuildScratchLayout l(n, a[1]);
      area("u32.idx0", l.idx0, n, 4);
      area("u32.idx1", l.idx1, n, 4);
      area("u32.flags", l.flags, n, 4);
      area("u32.table", l.table, a[1], 4);
      area("u32.chunk_tmp", l.chunk_tmp, num_chunks(std::max<size_t>(n, a[1])), 4);
      area("u32.starts", l.starts, n / 5 + 1, 4);
      area("u32.counters", l.counters, kNdtBuildCounters, 4);
      total("u32", l.size, 4);
    } else if (name == "grid") {
      const uint32_t count = static_cast<uint32_t>(a[0]);
      const NdtGridOffsetsLayout l(count);
      area("u32.offsets", l.offsets, count, 4);
      area("u32.chunk_tmp", l.chunk_tmp, num_chunks(count), 4);
      area("u32.total", l.total, 1, 4);
      total("u32", l.size, 4);
    } else if (name == "block") {  // a list in one block of bytes: the three areas' heads in units of their own elements
      const CellListLayout l(a[0]);
      if (l.u64_byte % 8 || l.f64_byte % 8 || l.u32_byte % 4) return 3;
      cell_list(l, "block", l.u64_byte / 8, "block", l.f64_byte / 8, "block", l.u32_byte / 4);
      total("block", l.bytes, 1);
    } else if (name == "cluster") {
      const ClusterLayout l(a[0], a[1]);
      area("f64.table_wsum", l.table_wsum, a[0], 8);
      area("u32.table_count", l.table_count, a[0], 4);
      area("u32.table_cluster", l.table_cluster, a[0], 4);
      cell_list(l.list, "u64", l.list_u64, "f64", l.list_f64, "u32", l.list_u32);
      total("f64", l.f64_size, 8);
      total("u32", l.u32_size, 4);
      total("u64", l.u64_size, 8);
    } else if (name == "csums") {
      const ClusterSumsLayout l(static_cast<uint32_t>(a[0]), a[1]);
      area("sums.partials", l.partials, l.rows * num_chunks(a[1]), 8);
      area("sums.sums", l.sums, l.rows, 8);
      total("sums", l.size, 8);
    } else if (name == "comm") {
      const CommLayout l(a[0]);
      area("f64.scalars", l.scalars, kCommScalars, 8);
      area("f64.sums", l.sums, a[0], 8);
      area("f64.stats", l.stats, a[0] * kStatsRecord, 8);
      area("f64.intervals", l.intervals, 2 * a[0], 8);
      area("f64.estimates", l.estimates, a[0] * kEstRecord, 8);
      total("f64", l.f64_size, 8);
      area("i64.counts", l.counts, a[0], 8);
      area("i64.gathered", l.gathered, a[0] * a[0], 8);
      total("i64", l.i64_size, 8);
    } else if (name == "commhost") {
      const CommHostLayout l;
      area("host.doubles", l.doubles, l.words, 8);
      area("host.words", l.words, l.size - l.words, 8);
      total("host", l.size, 8);
    } else return 2;
    std::printf("\n");
  }
  return 0;
}
"""

CAPACITIES = (1, 255, 256, 257, 1023, 1024, 1025, 4096, 262143, 262144, 262145, 1_000_000, 10_000_000)
WORLDS = (1, 2, 3, 64)
NDT_POINTS = (1, 4, 5, 6, 1000)
GRID_CELLS = (1, 256, 257)
ROUTE_M = (0, 1, 3, 4, 5, 256, 257)


def chunks(n):
    return (n + 2047) // 2048


def table_capacities(cap):
    """1024, and ensure_kld's: the power of two, at least 1024, that is not below 2 * cap."""
    tc = 1024
    while tc < 2 * cap:
        tc <<= 1
    return sorted({1024, tc})


def round4(c):
    return (c + 3) & ~3


CASES = {
    "sort": ["sort:%d" % c for c in CAPACITIES],
    "chunk": ["chunk:%d" % c for c in CAPACITIES],
    "kld": ["kld:%d" % c for c in CAPACITIES],
    "est": ["est:%d" % c for c in (0,) + CAPACITIES],
    "draw": ["draw:%d" % c for c in CAPACITIES],
    "xchg": ["xchg:%d,%d" % (m, w) for m in (0, 1, 255, 4096) for w in WORLDS],
    "ndtw": ["ndtw:%d" % n for n in NDT_POINTS],
    "lfw": ["lfw:%d" % c for c in CAPACITIES + (447, 448, 449)],
    "route": ["route:%d,%d" % (w, m) for w in WORLDS for m in ROUTE_M + CAPACITIES],
    "ndt": ["ndt:%d,%d" % (n, 256 * chunks(n)) for n in NDT_POINTS + (2048, 2049, 1_000_000)],  # (ndt_radix_table_words: 256 per chunk)
    "grid": ["grid:%d" % c for c in GRID_CELLS + (2048, 2049)],
    "block": ["block:%d" % c for c in sorted({round4(c) for c in CAPACITIES} | {16384})],  # (16384: kHostCells)
    "cluster": ["cluster:%d,%d" % (t, c) for c in CAPACITIES for t in table_capacities(c)],
    "csums": ["csums:%d,%d" % (r, n) for r in (1, 3, 8) for n in CAPACITIES],
    "comm": ["comm:%d" % w for w in WORLDS],
    "commhost": ["commhost"],
}


def parent(case):
    """(areas: name -> byte offset, sizes: buffer -> bytes) as the code before scratch_layout.h computed them."""
    kind, _, rest = case.partition(":")
    a = [int(v) for v in rest.split(",")] if rest else []
    if kind == "sort":
        cap, nb = a[0], chunks(a[0])
        totals = 2 * cap + 1024 * nb  # s.table + kSortDigits * nblocks
        return ({"u32.keys": 0, "u32.perm": 4 * cap, "u32.table": 4 * 2 * cap, "u32.totals": 4 * totals,
                 "u32.bases": 4 * (totals + 1024),       # sort->totals + kSortDigits
                 "u32.flags": 4 * (totals + 1024 + 1024),  # bases[kSortDigits]
                 "u64.keyidx": 0, "f64.frame": 0, "f64.bbox": 8 * 8,
                 "f64.bbox_partials": 8 * (8 + 8),       # sort->bbox + 8
                 "f64.partial": 8 * (8 + 8 + 6 * nb)},   # s.bbox + 8 + 6 * nblocks
                {"u32": 4 * (2 * cap + 1024 * nb + 2 * 1024 + 16), "u64": 8 * cap,
                 "f64": 8 * (8 + 8 + 6 * (nb + 1) + 16 * min(cap, 262144))})
    if kind in ("chunk", "kld", "est", "draw", "xchg", "ndtw"):
        rows, stride, el, buf = {"chunk": (12, chunks(a[0]) + 1, 8, "chunk"), "kld": (2, chunks(a[0]) + 1, 4, "uchunk"),
                                 "est": (9, max(chunks(a[0]), 1), 8, "est"), "draw": (9, (a[0] + 1023) // 1024, 8, "partials"),
                                 "xchg": ((a[1] if len(a) > 1 else 0) + 1, 7 * a[0], 8, "exchange"), "ndtw": (2, a[0], 8, "words")}[kind]
        size = {"xchg": 7 * a[0] * ((a[1] if len(a) > 1 else 0) + 1)}.get(kind, rows * stride)
        areas = {"%s.row%d" % (buf, k): el * k * stride for k in range(rows)}
        if kind == "xchg":  # d_send = ptr, d_recv = d_send + kCellRecordDoubles * widest: the rows behind the first are one area
            areas = {"exchange.row0": 0, "exchange.row1": 8 * 7 * a[0]}
        return areas, {buf: el * size}
    if kind == "lfw":
        return {}, {"wsum": 8 * (a[0] // 448 + 2)}
    if kind == "route":
        world, m = a
        hist = world * chunks(m)
        per = hist // 2048 + 1
        return ({"u32.block_hist": 0, "u32.chunk_sum": 4 * hist, "u32.chunk_off": 4 * (hist + per), "u32.dest": 4 * (hist + 2 * per)},
                {"u32": 4 * (hist + 2 * (hist // 2048 + 1) + (m + 3) // 4 + 4)})
    if kind == "ndt":
        n, table = a
        ch, starts = chunks(max(n, table)), n // 5 + 1
        return ({"u32.idx0": 0, "u32.idx1": 4 * n, "u32.flags": 4 * 2 * n, "u32.table": 4 * 3 * n, "u32.chunk_tmp": 4 * (3 * n + table),
                 "u32.starts": 4 * (3 * n + table + ch), "u32.counters": 4 * (3 * n + table + ch + starts)},
                {"u32": 4 * (3 * n + table + ch + starts + 7)})
    if kind == "grid":
        count = a[0]
        return ({"u32.offsets": 0, "u32.chunk_tmp": 4 * count, "u32.total": 4 * (count + chunks(count))}, {"u32": 4 * (count + chunks(count) + 1)})
    if kind == "block":
        c = a[0]
        f64, u32 = 8 * c, 8 * c + 8 * 5 * c  # f64 = u64 + capacity; u32 = f64 + kListF64 * capacity
        return ({"block.key": 0, "block.wsum": f64, "block.state": f64 + 8 * c, "block.first": u32, "block.count": u32 + 4 * c,
                 "block.slot": u32 + 4 * 2 * c, "block.cluster": u32 + 4 * 3 * c, "block.size": u32 + 4 * 4 * c},
                {"block": c * (8 + 5 * 8 + 4 * 4) + 64})
    if kind == "cluster":
        t, cap = a
        c = round4(cap)  # the device list's capacity: it was the particle capacity itself (the module's docstring: the one place an area moves)
        return ({"f64.table_wsum": 0, "u32.table_count": 0, "u32.table_cluster": 4 * t, "u64.key": 0, "f64.wsum": 8 * t, "f64.state": 8 * (t + c),
                 "u32.first": 4 * 2 * t, "u32.count": 4 * (2 * t + c), "u32.slot": 4 * (2 * t + 2 * c), "u32.cluster": 4 * (2 * t + 3 * c),
                 "u32.size": 4 * (2 * t + 4 * c)},
                {"f64": 8 * (t + 5 * cap), "u32": 4 * (2 * t + 4 * cap + 4), "u64": 8 * cap})
    if kind == "csums":
        rows = a[0] * 9
        partials = rows * chunks(a[1])
        return {"sums.partials": 0, "sums.sums": 8 * partials}, {"sums": 8 * (partials + rows)}
    if kind == "comm":
        w = a[0]
        return ({"f64.scalars": 0, "f64.sums": 8 * 20, "f64.stats": 8 * (20 + w), "f64.intervals": 8 * (20 + w * (1 + 3)),
                 "f64.estimates": 8 * (20 + w * (1 + 3 + 2)), "i64.counts": 0, "i64.gathered": 8 * w},
                {"f64": 8 * (20 + w * 16), "i64": 8 * (w + w * w)})
    if kind == "commhost":
        return {"host.doubles": 0, "host.words": 8 * (20 + 64 * 16)}, {"host": 8 * (20 + 64 * 16 + 64 * 64 + 64)}
    raise AssertionError(case)


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    """case -> (areas: name -> (byte offset, byte length, alignment), sizes: buffer -> bytes), every case of CASES from one run."""
    d = tmp_path_factory.mktemp("scratch_layout")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "beluga_amd", "csrc"), str(src), "-o", str(exe)])
    cases = [c for kind in CASES.values() for c in kind]
    out = subprocess.check_output([str(exe)] + cases, text=True).splitlines()
    assert len(out) == len(cases)
    parsed = {}
    for case, line in zip(cases, out):
        words = line.split("|")
        assert words[0] == case
        areas, sizes = {}, {}
        for w in words[1:]:
            f = w.split(",")
            if f[0].startswith("="):
                sizes[f[0][1:]] = int(f[1])
            else:
                areas[f[0]] = tuple(int(v) for v in f[1:])
        parsed[case] = (areas, sizes)
    return parsed


def buffer_of(area):
    return area.split(".")[0]


KINDS = sorted(CASES)


@pytest.mark.parametrize("kind", KINDS)
def test_the_areas_of_a_buffer_are_disjoint_and_end_inside_it(layouts, kind):
    for case in CASES[kind]:
        areas, sizes = layouts[case]
        spans = sorted((off, off + length, name) for name, (off, length, _) in areas.items())
        for name, (off, length, _) in areas.items():
            assert off + length <= sizes[buffer_of(name)], (case, name)
        for buf in sizes:
            mine = [s for s in spans if buffer_of(s[2]) == buf]
            for (_, end, first), (start, _, second) in zip(mine, mine[1:]):
                assert end <= start, (case, first, second)


@pytest.mark.parametrize("kind", KINDS)
def test_no_buffer_is_smaller_than_it_was(layouts, kind):
    for case in CASES[kind]:
        _, sizes = layouts[case]
        _, before = parent(case)
        assert set(sizes) == set(before), case
        for buf, size in sizes.items():
            assert size >= before[buf], (case, buf)


@pytest.mark.parametrize("kind", KINDS)
def test_every_area_lies_where_it_lay(layouts, kind):
    for case in CASES[kind]:
        areas, _ = layouts[case]
        before, _ = parent(case)
        named = {name: off for name, (off, _, _) in areas.items() if name in before}
        assert named == before, case  # (areas the parent had no name for - slack, the spare row - are held by the two tests above)


@pytest.mark.parametrize("kind", KINDS)
def test_every_area_is_aligned_to_its_element(layouts, kind):
    """(the cell list's states: 16 bytes, which is why a list's capacity is a multiple of 4 - the module's docstring)"""
    off_boundary = [(case, name, off % align) for case in CASES[kind] for name, (off, _, align) in layouts[case][0].items() if off % align]
    assert off_boundary == []


def test_the_device_list_moves_only_for_capacities_that_are_no_multiple_of_4(layouts):
    """Against the earlier expressions at the PARTICLE capacity: nothing moves where that is a multiple of 4; elsewhere the first area of
    each type stays, the areas behind it move back by the rounding times the arrays before them, and the states that lay off a 16-byte
    boundary (odd capacities) no longer do."""
    for case in CASES["cluster"]:
        t, cap = (int(v) for v in case.split(":")[1].split(","))
        pad = round4(cap) - cap
        areas = {name: off for name, (off, _, _) in layouts[case][0].items()}
        was = {"f64.table_wsum": 0, "u32.table_count": 0, "u32.table_cluster": 4 * t, "u64.key": 0, "f64.wsum": 8 * t, "f64.state": 8 * (t + cap),
               "u32.first": 4 * 2 * t, "u32.count": 4 * (2 * t + cap), "u32.slot": 4 * (2 * t + 2 * cap), "u32.cluster": 4 * (2 * t + 3 * cap),
               "u32.size": 4 * (2 * t + 4 * cap)}
        arrays_before = {"f64.state": 1, "u32.count": 1, "u32.slot": 2, "u32.cluster": 3, "u32.size": 4}
        element = {"f64": 8, "u32": 4, "u64": 8}
        for name, off in was.items():
            assert areas[name] == off + element[buffer_of(name)] * pad * arrays_before.get(name, 0), (case, name)
        assert (was["f64.state"] % 16 != 0) == (cap % 2 == 1) and areas["f64.state"] % 16 == 0, case
        assert pad == 0 or cap % 4 != 0


def test_the_parameter_grid_is_the_agreed_one():
    assert len(CASES["sort"]) == 13 and len(CASES["route"]) == 4 * (7 + 13)
    assert len(CASES["cluster"]) == 13 + 9  # (two table capacities each, one where 2 * cap <= 1024: 1, 255, 256, 257)
    assert all(int(c.split(":")[1]) % 4 == 0 for c in CASES["block"])  # a block's capacity is a multiple of 4: the states are double4
