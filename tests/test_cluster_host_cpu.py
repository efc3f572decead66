"""The host pass of cluster_based_estimate (beluga_amd/csrc/cluster_host.cpp) on the CPU: a plain g++ compiles it with a short
driver that builds the occupied cells from particle states with the product's own spatial hash, runs the cluster assignment and
the merge of the shards' cell lists, and writes everything out.  The oracle's cluster_ids() (pinned by the reference's vectors
in test_oracle_golden.py) says what the ids have to be - exactly: ids are handed out in pop order, so a flood fill that visits
the cells in another order gives other ids even where the partition is the same."""
import math
import os
import subprocess

import numpy as np
import pytest

from beluga_amd import synth
from oracle import binding as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
// driver <in> <out> <linear> <angular> <percentile> [cut_0 ... cut_W]
// in: n records of (cos, sin, x, y, weight).  out, in 8-byte words: winner (-1: none), C, the cell of every particle [n],
// the cluster of every cell [C], the cells [C][7]; with cuts (the bounds of W contiguous shards) also: M, the merged cells [M][7],
// and 1 if every rank found each of its cells at the index the merge reported (0 otherwise).
#include <cstdio>
#include <cstdlib>
#include <unordered_map>
#include <vector>

#include "cluster_host.h"

using namespace mcl;

static std::vector<ClusterCell> cells_of(const std::vector<double>& p, size_t begin, size_t end, double lin, double ang,
                                         std::vector<long long>* cell_of_particle) {
  std::vector<ClusterCell> cells;
  std::unordered_map<unsigned long long, size_t> at;
  for (size_t i = begin; i < end; ++i) {
    const Pose2 s{Rot2{p[5 * i], p[5 * i + 1]}, p[5 * i + 2], p[5 * i + 3]};
    const unsigned long long key = host_cell_key(s, lin, ang);
    const auto found = at.try_emplace(key, cells.size());
    if (found.second) cells.push_back(ClusterCell{key, 0.0, 0, s});
    cells[found.first->second].weight_sum += p[5 * i + 4];
    cells[found.first->second].count += 1;
    if (cell_of_particle) cell_of_particle->push_back(static_cast<long long>(found.first->second));
  }
  return cells;
}

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  std::fseek(in, 0, SEEK_END);
  const size_t n = static_cast<size_t>(std::ftell(in)) / (5 * sizeof(double));
  std::fseek(in, 0, SEEK_SET);
  std::vector<double> p(5 * n);
  if (std::fread(p.data(), sizeof(double), p.size(), in) != p.size()) return 2;
  std::fclose(in);
  const double lin = std::atof(argv[3]), ang = std::atof(argv[4]), pct = std::atof(argv[5]);

  std::vector<long long> cell_of_particle;
  const std::vector<ClusterCell> cells = cells_of(p, 0, n, lin, ang, &cell_of_particle);
  const ClusterAssignment a = assign_clusters(cells, lin, ang, pct);
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  auto word = [out](long long v) { std::fwrite(&v, sizeof v, 1, out); };
  word(a.winner ? static_cast<long long>(*a.winner) : -1);
  word(static_cast<long long>(cells.size()));
  std::fwrite(cell_of_particle.data(), sizeof(long long), n, out);
  for (const unsigned int c : a.cluster_of_cell) word(c);
  std::fwrite(cells.data(), sizeof(ClusterCell), cells.size(), out);

  if (argc > 7) {  // every shard's cells, packed to the widest list as the ranks send them, then merged
    const uint32_t world = static_cast<uint32_t>(argc - 7);
    std::vector<std::vector<ClusterCell>> shard(world);
    std::vector<uint64_t> count_of(world);
    size_t widest = 0;
    for (uint32_t r = 0; r < world; ++r) {
      shard[r] = cells_of(p, std::strtoull(argv[6 + r], nullptr, 10), std::strtoull(argv[7 + r], nullptr, 10), lin, ang, nullptr);
      count_of[r] = shard[r].size();
      widest = shard[r].size() > widest ? shard[r].size() : widest;
    }
    std::vector<ClusterCell> gathered(widest * world, ClusterCell{});
    for (uint32_t r = 0; r < world; ++r)
      for (size_t j = 0; j < shard[r].size(); ++j) gathered[r * widest + j] = shard[r][j];
    const std::vector<ClusterCell> merged = merge_cluster_cells(gathered.data(), widest, count_of.data(), world);
    long long indices_right = 1;
    for (uint32_t r = 0; r < world; ++r) {
      std::vector<uint32_t> index;
      const std::vector<ClusterCell> again = merge_cluster_cells(gathered.data(), widest, count_of.data(), world, r, &index);
      if (again.size() != merged.size() || index.size() != shard[r].size()) indices_right = 0;
      for (size_t j = 0; indices_right && j < index.size(); ++j)
        if (index[j] >= merged.size() || merged[index[j]].key != shard[r][j].key) indices_right = 0;
    }
    word(static_cast<long long>(merged.size()));
    std::fwrite(merged.data(), sizeof(ClusterCell), merged.size(), out);
    word(indices_right);
  }
  std::fclose(out);
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("cluster_host")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    csrc = os.path.join(ROOT, "beluga_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", csrc, "-I", os.path.join(ROOT, "include"), str(src),
                           os.path.join(csrc, "cluster_host.cpp"), "-o", str(exe)])
    return str(exe), d


def _run(driver, states, w, res, cuts=()):
    exe, d = driver
    n = len(w)
    np.concatenate([np.asarray(states, dtype=np.float64).reshape(n, 4), np.asarray(w, dtype=np.float64).reshape(n, 1)],
                   axis=1).tofile(str(d / "in.bin"))
    subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")] + [repr(float(v)) for v in res] + [str(int(c)) for c in cuts])
    words = np.fromfile(str(d / "out.bin"), dtype=np.int64)
    winner, cells = int(words[0]), int(words[1])
    at = 2
    out = {"winner": None if winner < 0 else winner, "cell_of_particle": words[at:at + n]}
    at += n
    out["cluster_of_cell"] = words[at:at + cells]
    at += cells
    out["cells"] = words[at:at + 7 * cells].reshape(cells, 7)
    at += 7 * cells
    if cuts:
        merged = int(words[at])
        out["merged"] = words[at + 1:at + 1 + 7 * merged].reshape(merged, 7)
        out["indices_right"] = int(words[at + 1 + 7 * merged])
        at += 2 + 7 * merged
    assert at == len(words)
    return out


def _multicluster(xmin, xmax, ymin, ymax, step):  # the data set of test_oracle_golden.py (test_cluster_based_estimation.cpp:67-94)
    xw, yw = xmax - xmin, ymax - ymin
    states, weights = [], []
    x = step / 2.0
    while x <= xw:
        y = step / 2.0
        while y <= yw:
            k = (0.0 if 2 * x < xw else 1.0) + (0.0 if 2 * y < yw else 2.0) + 1.0
            wt = abs(math.sin(2.0 * math.pi * x / xw)) * abs(math.sin(2.0 * math.pi * y / yw)) * k
            states.append(orc.se2(x + xmin, y + ymin, 0.0))
            weights.append(max(0.0, wt - k / 2.0))
            y += step
        x += step
    return np.array(states), np.array(weights)


def _bimodal(n, weights="gamma"):  # the cloud of test_gpu_parity.py::test_cluster_based_estimate_bimodal_cloud_and_update_path
    a = synth.normal_particles(int(n * 0.6), (2.0, 1.0, 0.5), (0.3, 0.3, 0.15), seed=1)
    b = synth.normal_particles(n - len(a), (-4.0, -3.0, -2.0), (0.3, 0.3, 0.15), seed=2)
    states = np.concatenate([a, b])[np.random.Generator(np.random.MT19937(3)).permutation(n)]
    rng = np.random.Generator(np.random.MT19937(4))
    if weights == "gamma":
        return states, rng.gamma(2.0, 1.0, n)
    return states, rng.integers(0, 1024, n) / 1024.0  # multiples of 2^-10 below 1: every sum of them is exact


DEFAULTS = (0.2, 0.524, 0.9)
# (cov_rtol, cov_atol): what test_gpu_parity.py asks of the same comparison on the same sets
CASES = {
    "multicluster_coarse": (lambda: _multicluster(0.0, 36.0, 0.0, 36.0, 1.0), (1.0, math.pi / 2.0, 0.9), (1e-8, 1e-11)),
    "multicluster_fine": (lambda: _multicluster(-2.0, 2.0, -2.0, 2.0, 0.025), DEFAULTS, (1e-8, 1e-11)),
    "bimodal": (lambda: _bimodal(200_000), DEFAULTS, (1e-7, 1e-10)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_cluster_ids_and_winner_are_the_references(driver, case):
    make, res, (cov_rtol, cov_atol) = CASES[case]
    states, w = make()
    got = _run(driver, states, w, res)
    want_ids = orc.cluster_ids(states, w, *res).astype(np.int64)
    ids = got["cluster_of_cell"][got["cell_of_particle"]]
    assert np.array_equal(ids, want_ids)
    # the reference's choice (estimate_clusters :345-411): clusters of more than one particle, the first one of maximum total weight,
    # the totals added up in cell order
    cell, first = np.unique(got["cell_of_particle"], return_index=True)
    assert np.array_equal(cell, np.arange(len(got["cells"]))) and np.all(np.diff(first) > 0)  # first-occurrence order
    cell_ids = want_ids[first]
    wsum, count = got["cells"][:, 1].view(np.float64), got["cells"][:, 2]
    assert np.array_equal(count, np.bincount(got["cell_of_particle"]))
    total_w, total_n = np.zeros(cell_ids.max() + 1), np.zeros(cell_ids.max() + 1, dtype=np.int64)
    for k in range(len(cell_ids)):
        total_w[cell_ids[k]] += wsum[k]
        total_n[cell_ids[k]] += count[k]
    best = None
    for c in range(len(total_w)):
        if total_n[c] > 1 and (best is None or total_w[best] < total_w[c]):
            best = c
    assert best is not None and got["winner"] == best
    sel = ids == got["winner"]
    pose, cov = orc.estimate(states[sel], w[sel])
    want_pose, want_cov = orc.cluster_based_estimate(states, w, *res)
    np.testing.assert_allclose(pose, want_pose, atol=1e-9)
    np.testing.assert_allclose(cov, want_cov, rtol=cov_rtol, atol=cov_atol)


def test_no_cluster_of_more_than_one_particle_is_no_winner(driver):
    far = np.array([orc.se2(-10, -10, 0), orc.se2(-10, 10, 0), orc.se2(10, -10, 0), orc.se2(10, 10, 0)])  # NightmareDistributionTest
    got = _run(driver, far, np.full(4, 0.2), DEFAULTS)
    assert got["winner"] is None
    assert len(got["cells"]) == 4 and np.array_equal(got["cells"][:, 2], np.ones(4, dtype=np.int64))
    assert np.array_equal(got["cluster_of_cell"][got["cell_of_particle"]], orc.cluster_ids(far, np.full(4, 0.2)).astype(np.int64))


N_MERGE = 30_000
SHARDS = {
    "2": (0, N_MERGE // 2, N_MERGE),
    "3": (0, N_MERGE // 3, 2 * (N_MERGE // 3), N_MERGE),
    "3_one_empty": (0, N_MERGE // 3, N_MERGE // 3, N_MERGE),
    "4": (0, N_MERGE // 4, N_MERGE // 2, 3 * (N_MERGE // 4), N_MERGE),
    "4_first_empty": (0, 0, N_MERGE // 4, 3 * (N_MERGE // 4), N_MERGE),
}


@pytest.mark.parametrize("weights", ["gamma", "exact"])
@pytest.mark.parametrize("shards", sorted(SHARDS))
def test_merged_shard_lists_are_the_one_list(driver, shards, weights):
    """Contiguous shards' cells, packed and merged in rank order, are the whole set's cells: keys, order, counts and
    representative states bit for bit; the weight sums too where every partial sum is exact (weights that are multiples of
    2^-10 below 1: a sum of 30 000 of them needs 25 bits), so that the order of the additions cannot matter."""
    states, w = _bimodal(N_MERGE, weights)
    got = _run(driver, states, w, DEFAULTS, SHARDS[shards])
    one, merged = got["cells"], got["merged"]
    assert got["indices_right"] == 1
    assert merged.shape == one.shape and len(one) > 100
    assert np.array_equal(merged[:, 0], one[:, 0])    # keys, in order
    assert np.array_equal(merged[:, 2], one[:, 2])    # counts
    assert np.array_equal(merged[:, 3:], one[:, 3:])  # states (bit patterns)
    if weights == "exact":
        assert np.array_equal(merged[:, 1], one[:, 1])
