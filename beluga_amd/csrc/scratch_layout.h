// scratch_layout.h — the layout of every scratch buffer that holds several arrays behind one another.  One struct per buffer (or group
// of buffers sized together), built from the parameters its size depends on: each area is a member, an ELEMENT offset into its buffer,
// and the element count for ensure() is a member of the same struct - both come out of one running sum (Cursor), so they cannot
// disagree.  This header is the only place that says where an area lies; context.hip turns the offsets into pointers.
// Plain C++17, no HIP (tests/test_scratch_layout_cpu.py holds every offset to a literal table).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace mcl {

// Deterministic chunked reductions / scans.  Chunk = 2048 consecutive elements per workgroup.
constexpr uint32_t kChunk = 2048;
inline uint32_t num_chunks(uint64_t n) { return static_cast<uint32_t>((n + kChunk - 1) / kChunk); }

// take(count): the offset of the next area of `count` elements; `at` is the size of everything taken so far.
struct Cursor {
  size_t at = 0;
  size_t take(size_t count) {
    const size_t offset = at;
    at += count;
    return offset;
  }
};

// `rows` arrays of `stride` elements each, row k at k * stride.
struct RowsLayout {
  size_t rows = 0, stride = 0;
  size_t row(size_t k) const { return k * stride; }
  size_t size() const { return rows * stride; }
};
// d_chunk: the twelve rows of per-chunk partial sums of the reductions and scans (mcl_ctx::chunk_row).
constexpr size_t kChunkRows = 12;
constexpr size_t kChunkRowSlack = 1;  // one element per row beyond num_chunks(cap): slack kept from before
inline RowsLayout chunk_rows(uint64_t cap) { return RowsLayout{kChunkRows, num_chunks(cap) + kChunkRowSlack}; }
// d_uchunk: the KLD scan's two rows of chunk sums over `cap` candidates (the same stride as d_chunk's).
inline RowsLayout kld_chunk_rows(uint64_t cap) { return RowsLayout{2, num_chunks(cap) + kChunkRowSlack}; }
// d_ndt_est: the nine rows of estimate partials per chunk of n particles (launch_estimate_sums); never empty.
inline RowsLayout estimate_rows(uint64_t n) { return RowsLayout{9, std::max<uint32_t>(num_chunks(n), 1u)}; }
// d_est_partials: the nine rows the draw kernel leaves, one element per draw workgroup (1024 candidates).
inline RowsLayout draw_estimate_rows(uint64_t max_particles) { return RowsLayout{9, static_cast<size_t>((max_particles + 1023) / 1024)}; }
// d_cell_exchange: row 0 = this rank's cell records, padded to the widest rank's count; rows 1 .. world = the gathered records of all ranks.
inline RowsLayout cell_exchange_rows(size_t record_doubles, uint64_t widest, uint32_t world) {
  return RowsLayout{static_cast<size_t>(world) + 1, record_doubles * static_cast<size_t>(widest)};
}
// The NDT build's 64-bit key words: the sort's ping and pong lists of n words (NdtBuildScratch::words).
inline RowsLayout ndt_word_rows(uint32_t n) { return RowsLayout{2, n}; }

// d_lf_wsum: one sum per workgroup of the LF patch kernel, which takes kLfPatchParticles particles (seven waves; kernels.hip kPatchParticles).
constexpr uint64_t kLfPatchParticles = 448;
constexpr size_t kLfWeightSumsSlack = 1;  // slack kept from before
inline size_t lf_weight_sums_size(uint64_t cap) {
  return static_cast<size_t>(cap / kLfPatchParticles) + 1 /* the last, partly filled workgroup */ + kLfWeightSumsSlack;
}

// ---- spatial ordering (SortScratch, kernels.h): d_sort_u32, d_sort_u64, d_sort_f64 ---------------------------------------------------
constexpr uint32_t kSortDigits = 1024;  // two least-significant-digit-first passes of 10 bits each
constexpr uint32_t kLfMaxSegments = 16;
constexpr uint64_t kLfSegmentedBelow = 262144;  // particles
constexpr size_t kSortFlagWords = 16;  // behind the bases: word 0 = "some bucket is beyond kSortHugeBucket" (k_sort_buckets reads bases[kSortDigits]), the rest unused
constexpr size_t kKeyFrameDoubles = 8;  // the device-resident KeyFrame's room at the head of d_sort_f64
struct SortLayout {
  size_t nblocks;                                              // chunks of `cap` particles
  size_t keys, perm, table, totals, bases, flags, u32_size;    // d_sort_u32: [cap] [cap] [kSortDigits][nblocks] [kSortDigits] [kSortDigits] [16]
  size_t keyidx, u64_size;                                     // d_sort_u64: [cap]
  size_t frame, bbox, bbox_partials, partial, spare_row, f64_size;  // d_sort_f64: [8] [8] [6][nblocks] [kLfMaxSegments][min(cap, 262144)] [6]
  explicit SortLayout(uint64_t cap) : nblocks(num_chunks(cap)) {
    Cursor u32, u64, f64;
    keys = u32.take(cap);
    perm = u32.take(cap);
    table = u32.take(static_cast<size_t>(kSortDigits) * nblocks);
    totals = u32.take(kSortDigits);
    bases = u32.take(kSortDigits);
    flags = u32.take(kSortFlagWords);
    u32_size = u32.at;
    keyidx = u64.take(cap);
    u64_size = u64.at;
    frame = f64.take(kKeyFrameDoubles);
    bbox = f64.take(8);
    bbox_partials = f64.take(6 * nblocks);
    partial = f64.take(kLfMaxSegments * static_cast<size_t>(std::min<uint64_t>(cap, kLfSegmentedBelow)));
    spare_row = f64.take(6);  // the size used to count d_chunk's stride (num_chunks + 1) rows of bounding-box partials, the carve num_chunks: the larger is kept
    f64_size = f64.at;
  }
};

// ---- sharded resampling: d_route_u32, the scratch of launch_route_targets over m targets and `world` shards ---------------------------
constexpr size_t kRouteSlackWords = 4;  // slack kept from before
struct RouteLayout {
  size_t hist;                                                  // world * num_chunks(m) block histograms
  size_t block_hist, chunk_sum, chunk_off, dest, slack, size;   // u32 words; dest: m bytes (the owning shard of every target), in whole words
  RouteLayout(uint32_t world, uint64_t m) : hist(static_cast<size_t>(world) * num_chunks(m)) {
    Cursor c;
    block_hist = c.take(hist);
    chunk_sum = c.take(hist / kChunk + 1);
    chunk_off = c.take(hist / kChunk + 1);
    dest = c.take(static_cast<size_t>((m + 3) / 4));
    slack = c.take(kRouteSlackWords);
    size = c.at;
  }
};

// ---- NDT map build (NdtBuildScratch, kernels.h): the u32 scratch over n points; `table` = ndt_radix_table_words(n) ----------------------
constexpr uint32_t kNdtBuildCounters = 7;  // NdtBuildCounter (kernels.h)
struct NdtBuildScratchLayout {
  size_t idx0, idx1, flags, table, chunk_tmp, starts, counters, size;
  NdtBuildScratchLayout(uint32_t n, size_t table_words) {
    Cursor c;
    idx0 = c.take(n);
    idx1 = c.take(n);
    flags = c.take(n);
    table = c.take(table_words);
    chunk_tmp = c.take(num_chunks(std::max<size_t>(n, table_words)));
    starts = c.take(n / 5 + 1);  // a kept cell has 5 points or more
    counters = c.take(kNdtBuildCounters);
    size = c.at;
  }
};
// launch_ndt_grid_offsets over `count` grid cells: the offsets, their scan's chunk sums, the number of occupied cells.
struct NdtGridOffsetsLayout {
  size_t offsets, chunk_tmp, total, size;
  explicit NdtGridOffsetsLayout(uint32_t count) {
    Cursor c;
    offsets = c.take(count);
    chunk_tmp = c.take(num_chunks(count));
    total = c.take(1);
    size = c.at;
  }
};

// ---- cluster cells (CellTable, CellList: kernels.h) -------------------------------------------------------------------------------------
// A CellList of `capacity` cells and, behind it, the cells' cluster ids, laid over one area per element type:
//   u64: key[c] | f64: wsum[c], state[4 c] | u32: first[c], count[c], slot[c], cluster[c], size
// The offsets count from the head of the list's area of that type.  The same description serves the device arrays (ClusterLayout: one
// area in each of d_cell_u64 / d_cell_f64 / d_cell_u32) and a list in ONE block of bytes (the mapped host list, the host's copy of a
// large list): there the three areas lie behind one another at u64_byte / f64_byte / u32_byte.  A list's capacity is a multiple of 4
// (cell_list_capacity): the double4 states lie `capacity` doubles behind an aligned head, and 4 doubles are their 32 bytes.
inline size_t cell_list_capacity(uint64_t cells) { return (static_cast<size_t>(cells) + 3) & ~static_cast<size_t>(3); }
constexpr size_t kCellListSizeWords = 4;  // the list's size, one word, in a 16-byte granule of its own (three words of slack kept from before)
constexpr size_t kCellBlockSlackBytes = 48;  // behind a block's size granule, up to a cache line: slack kept from before
struct CellListLayout {
  size_t capacity;
  size_t key, u64_size;
  size_t wsum, state, f64_size;  // state: double4 records, in doubles
  size_t first, count, slot, cluster, size_word, u32_size;
  size_t u64_byte, f64_byte, u32_byte, bytes;
  explicit CellListLayout(size_t cells) : capacity(cells) {
    Cursor u64, f64, u32, block;
    key = u64.take(capacity);
    u64_size = u64.at;
    wsum = f64.take(capacity);
    state = f64.take(4 * capacity);
    f64_size = f64.at;
    first = u32.take(capacity);
    count = u32.take(capacity);
    slot = u32.take(capacity);
    cluster = u32.take(capacity);
    size_word = u32.take(kCellListSizeWords);
    u32_size = u32.at;
    u64_byte = block.take(u64_size * sizeof(unsigned long long));
    f64_byte = block.take(f64_size * sizeof(double));
    u32_byte = block.take(u32_size * sizeof(unsigned int));
    block.take(kCellBlockSlackBytes);
    bytes = block.at;
  }
};
// d_cell_f64 / d_cell_u32 / d_cell_u64: the cell table's columns beside the KLD table's keys and first particles, `table_capacity` wide,
// then the device list, which holds the context's `capacity` cells and is laid out for cell_list_capacity(capacity): laid out for
// the capacity itself, an odd one used to leave the states 8 bytes off a 16-byte boundary.
struct ClusterLayout {
  CellListLayout list;
  size_t table_wsum, list_f64, f64_size;
  size_t table_count, table_cluster, list_u32, u32_size;
  size_t list_u64, u64_size;
  ClusterLayout(uint64_t table_capacity, uint64_t capacity) : list(cell_list_capacity(capacity)) {
    Cursor f64, u32, u64;
    table_wsum = f64.take(table_capacity);
    list_f64 = f64.take(list.f64_size);
    f64_size = f64.at;
    table_count = u32.take(table_capacity);
    table_cluster = u32.take(table_capacity);
    list_u32 = u32.take(list.u32_size);
    u32_size = u32.at;
    list_u64 = u64.take(list.u64_size);
    u64_size = u64.at;
  }
};
// d_cluster_sums (mcl_estimate_clusters): nine rows of per-chunk partials for each of `ranks` clusters, then their sums.
struct ClusterSumsLayout {
  size_t rows, partials, sums, size;
  ClusterSumsLayout(uint32_t ranks, uint64_t n) : rows(static_cast<size_t>(ranks) * 9) {
    Cursor c;
    partials = c.take(rows * num_chunks(n));
    sums = c.take(rows);
    size = c.at;
  }
};

// ---- shard communication: d_comm_f64, d_comm_i64, h_comm ---------------------------------------------------------------------------------
constexpr size_t kCommScalars = 20;                         // this rank's scalars at the head of d_comm_f64 (CommSlot, context.hip)
constexpr size_t kStatsRecord = 3, kEstRecord = 10;         // ShardStats; the nine estimate sums + the overflow flag
constexpr size_t kCommPerRank = 1 + kStatsRecord + 2 + kEstRecord, kMaxWorld = 64;  // doubles gathered per rank; ranks at most
struct CommLayout {
  size_t scalars, sums, stats, intervals, estimates, f64_size;  // d_comm_f64: [kCommScalars] | sums[world] | stats[world][kStatsRecord] | ends[world], offsets[world] | estimates[world][kEstRecord]
  size_t counts, gathered, i64_size;                            // d_comm_i64: counts[world] | gathered counts[world][world]
  explicit CommLayout(size_t world) {
    Cursor f64, i64;
    scalars = f64.take(kCommScalars);
    sums = f64.take(world);
    stats = f64.take(world * kStatsRecord);
    intervals = f64.take(2 * world);
    estimates = f64.take(world * kEstRecord);
    f64_size = f64.at;
    counts = i64.take(world);
    gathered = i64.take(world * world);
    i64_size = i64.at;
  }
};
// h_comm, in doubles: the device block's doubles as kMaxWorld ranks would need them (the global sum, the gathered statistics and the CDF
// intervals to upload lie at its head), then the 64-bit words of the counts' all-gathers, kMaxWorld + 1 rows.  One size for every world.
struct CommHostLayout {
  size_t doubles, words, size;
  CommHostLayout() {
    const CommLayout widest(kMaxWorld);
    Cursor c;
    doubles = c.take(widest.f64_size);
    words = c.take(widest.i64_size);
    size = c.at;
  }
};

// ---- mcl_likelihoods*: d_likelihoods, the call's own doubles - the caller's n poses (4 each), their n scores, the staged measurement ----
// The measurement lies first, rounded up to whole pose records: every area then starts at a multiple of 32 bytes (the kernels read the
// poses as double4 and the measurement as double2).  The device form takes the measurement area alone (n = 0).
struct LikelihoodsLayout {
  size_t measurement, poses, out, size;
  LikelihoodsLayout(uint64_t n, size_t measurement_doubles) {
    Cursor c;
    measurement = c.take((measurement_doubles + 3) / 4 * 4);
    poses = c.take(4 * static_cast<size_t>(n));
    out = c.take(static_cast<size_t>(n));
    size = c.at;
  }
};

// ---- beam skipping: d_beam_skip and h_beam_skip, the count's own doubles - the staged scan (x, y per point) and, behind it, the counts ----
// The counts are uint32, two to a double: the area is rounded up to whole doubles and starts at a multiple of 16 bytes (the points
// take an even number of doubles).  The same layout in device memory and in the pinned host block that stages one and receives the other.
struct BeamSkipLayout {
  size_t points, counts, size;
  explicit BeamSkipLayout(uint64_t num_points) {
    Cursor c;
    points = c.take(2 * static_cast<size_t>(num_points));
    counts = c.take((static_cast<size_t>(num_points) + 1) / 2);
    size = c.at;
  }
};

// ---- mcl_global_search*: d_search_f64, d_search_u64, d_search_u32 and the pinned h_search, the call's own ---------------------------------
// Sized by the chunk (`candidates` = SearchPlan::chunk_candidates, `cells` = its cells, `tiles` sort tiles of `tile` entries), never by
// the number of candidates of the map.
//   f64: the heading table (cos, sin per heading, rounded up to whole poses: the poses behind it are read as double4) | the chunk's
//        poses | its scores
//   u64: the chunk's ids | two sets of sorted runs (keys, ids: the tile sort's output and the merge levels' ping and pong) | the pool
//        (keys, ids), twice: a merge reads one and writes the other
//   u32: the chunk's selected cells | the count of them (one word in a granule of four)
//   h_search (pinned, 8-byte words): the heading table to upload | the final pool's keys and ids | the count word of a chunk
struct SearchLayout {
  size_t table, poses, scores, f64_size;
  size_t ids, run_keys[2], run_ids[2], pool_keys[2], pool_ids[2], u64_size;
  size_t selected, count, u32_size;
  size_t h_table, h_pool_keys, h_pool_ids, h_count, h_size;
  SearchLayout(uint32_t headings, size_t cells, size_t candidates, size_t tiles, size_t tile, size_t pool_capacity) {
    Cursor f64, u64, u32, host;
    table = f64.take((2 * static_cast<size_t>(headings) + 3) / 4 * 4);
    poses = f64.take(4 * candidates);
    scores = f64.take(candidates);
    f64_size = f64.at;
    ids = u64.take(candidates);
    for (int k = 0; k < 2; ++k) {
      run_keys[k] = u64.take(tiles * tile);
      run_ids[k] = u64.take(tiles * tile);
    }
    for (int k = 0; k < 2; ++k) {
      pool_keys[k] = u64.take(pool_capacity);
      pool_ids[k] = u64.take(pool_capacity);
    }
    u64_size = u64.at;
    selected = u32.take(cells);
    count = u32.take(4);
    u32_size = u32.at;
    h_table = host.take(2 * static_cast<size_t>(headings));
    h_pool_keys = host.take(pool_capacity);
    h_pool_ids = host.take(pool_capacity);
    h_count = host.take(1);
    h_size = host.at;
  }
};

// ---- mcl_local_search*: the call's own 8-byte words, in device memory and in the pinned block that stages one part and receives another ----
// device: off[] (2 Kx + 1) | the seeds' (x, y) | the rotation table (cos, sin per seed and step) - these three in the pinned block's
//   order, so that one copy uploads them - | a pass's poses | its scores | the results per seed: kLocalResultDoubles doubles, then
//   kLocalResultWords uint64.  Every area is rounded up to whole poses (the poses are read as double4, the tables as double2).
// pinned: the three tables to upload | the results read back (the device's two result areas, one copy).
// The tables and the results are sized by the seeds, the poses and scores by the pass (LocalPlan::pass_candidates), never by n * L.
struct LocalSearchLayout {
  size_t off, seed_xy, rot, tables_size, poses, scores, results_f64, results_u64, results_size, size;
  size_t h_tables, h_results, h_size;
  LocalSearchLayout(uint64_t seeds, uint32_t side_xy, uint32_t side_theta, uint64_t pass_candidates, size_t result_doubles, size_t result_words) {
    const auto whole = [](size_t doubles) { return (doubles + 3) / 4 * 4; };
    Cursor c, host;
    off = c.take(whole(side_xy));
    seed_xy = c.take(whole(2 * static_cast<size_t>(seeds)));
    rot = c.take(whole(2 * static_cast<size_t>(seeds) * side_theta));
    tables_size = c.at;
    poses = c.take(4 * static_cast<size_t>(pass_candidates));
    scores = c.take(whole(static_cast<size_t>(pass_candidates)));
    results_f64 = c.take(whole(result_doubles * static_cast<size_t>(seeds)));
    results_u64 = c.take(whole(result_words * static_cast<size_t>(seeds)));
    results_size = c.at - results_f64;
    size = c.at;
    h_tables = host.take(tables_size);
    h_results = host.take(results_size);
    h_size = host.at;
  }
};

// ---- mcl_cast_rays*: d_cast and the pinned h_cast, the call's own 8-byte words --------------------------------------------------------------
// d_cast: the bearing table (c, s per bearing, made into the far-end vectors in place; rounded up to whole poses: the poses behind it
// are read as double4) | the cell count, one word in a granule of four | a chunk's poses | its ranges | its hit cells (int64).  The
// device form takes the table and the count alone (chunk_poses = chunk_rays = 0); a call that wants no hit cells has no area for them.
// Sized by the chunk (CastPlan, raycast_host.h) and the table, never by the number of rays.
// h_cast: the bearings to upload | the cell count read back.
struct RayCastLayout {
  size_t table, count, poses, ranges, hits, size;
  size_t h_table, h_count, h_size;
  RayCastLayout(uint64_t num_bearings, uint64_t chunk_poses, uint64_t chunk_rays, bool hit_cells) {
    Cursor c, host;
    table = c.take((2 * static_cast<size_t>(num_bearings) + 3) / 4 * 4);
    count = c.take(4);
    poses = c.take(4 * static_cast<size_t>(chunk_poses));
    ranges = c.take(static_cast<size_t>(chunk_rays));
    hits = c.take(hit_cells ? static_cast<size_t>(chunk_rays) : 0);
    size = c.at;
    h_table = host.take(2 * static_cast<size_t>(num_bearings));
    h_count = host.take(1);
    h_size = host.at;
  }
};

}  // namespace mcl
