"""The host side of mcl_estimate_clusters (beluga_amd/csrc/cluster_host.cpp) on the CPU: the per-cluster totals assign_clusters hands
out and select_heaviest_clusters, the choice of the K clusters the device sums.  A plain g++ compiles both with a short driver, as
test_cluster_host_cpu.py does; the data sets are that file's, restated.  What the totals have to be comes from the oracle's
cluster_ids() and numpy sums over the particles: estimate_clusters (algorithm/cluster_based_estimation.hpp:337-399) keeps the clusters
of more than one particle, and the library reports the heaviest K of them by descending weight, ties by ascending id."""
import math
import os
import subprocess

import numpy as np
import pytest

from beluga_amd import synth
from oracle import binding as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
// driver set <in> <out> <linear> <angular> <percentile> k_0 k_1 ...
//   in: n records of (cos, sin, x, y, weight).  out, in 8-byte words: C clusters, weight[C] (doubles), count[C], then per k:
//   eligible, S = selected.size(), selected[S], rank_of_cluster[C] (-1: not selected)
// driver pick <in> <out> k_0 k_1 ...
//   in: C records of (weight, count as a double).  out: per k as above.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "cluster_host.h"

using namespace mcl;

static std::vector<double> read_doubles(const char* path) {
  std::vector<double> v;
  std::FILE* in = std::fopen(path, "rb");
  if (!in) std::exit(2);
  std::fseek(in, 0, SEEK_END);
  v.resize(static_cast<size_t>(std::ftell(in)) / sizeof(double));
  std::fseek(in, 0, SEEK_SET);
  if (std::fread(v.data(), sizeof(double), v.size(), in) != v.size()) std::exit(2);
  std::fclose(in);
  return v;
}

static void write_selection(std::FILE* out, const std::vector<double>& weight, const std::vector<uint64_t>& count, size_t k) {
  auto word = [out](long long v) { std::fwrite(&v, sizeof v, 1, out); };
  const ClusterSelection s = select_heaviest_clusters(weight, count, k);
  word(static_cast<long long>(s.eligible));
  word(static_cast<long long>(s.selected.size()));
  for (const unsigned int c : s.selected) word(c);
  if (s.rank_of_cluster.size() != weight.size()) std::exit(4);
  for (const unsigned int r : s.rank_of_cluster) word(r == kClusterNotSelected ? -1 : static_cast<long long>(r));
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const std::vector<double> p = read_doubles(argv[2]);
  std::FILE* out = std::fopen(argv[3], "wb");
  if (!out) return 2;
  auto word = [out](long long v) { std::fwrite(&v, sizeof v, 1, out); };
  if (std::strcmp(argv[1], "pick") == 0) {
    std::vector<double> weight;
    std::vector<uint64_t> count;
    for (size_t c = 0; c < p.size() / 2; ++c) {
      weight.push_back(p[2 * c]);
      count.push_back(static_cast<uint64_t>(p[2 * c + 1]));
    }
    for (int a = 4; a < argc; ++a) write_selection(out, weight, count, std::strtoull(argv[a], nullptr, 10));
    std::fclose(out);
    return 0;
  }
  if (argc < 7) return 2;
  const size_t n = p.size() / 5;
  const double lin = std::atof(argv[4]), ang = std::atof(argv[5]), pct = std::atof(argv[6]);
  std::vector<ClusterCell> cells;  // in first-occurrence order, as the library feeds them
  std::unordered_map<unsigned long long, size_t> at;
  for (size_t i = 0; i < n; ++i) {
    const Pose2 s{Rot2{p[5 * i], p[5 * i + 1]}, p[5 * i + 2], p[5 * i + 3]};
    const unsigned long long key = host_cell_key(s, lin, ang);
    const auto found = at.try_emplace(key, cells.size());
    if (found.second) cells.push_back(ClusterCell{key, 0.0, 0, s});
    cells[found.first->second].weight_sum += p[5 * i + 4];
    cells[found.first->second].count += 1;
  }
  const ClusterAssignment a = assign_clusters(cells, lin, ang, pct);
  if (a.weight.size() != a.count.size()) return 4;
  word(static_cast<long long>(a.weight.size()));
  std::fwrite(a.weight.data(), sizeof(double), a.weight.size(), out);
  for (const uint64_t c : a.count) word(static_cast<long long>(c));
  for (int k = 7; k < argc; ++k) write_selection(out, a.weight, a.count, std::strtoull(argv[k], nullptr, 10));
  std::fclose(out);
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("cluster_modes")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    csrc = os.path.join(ROOT, "beluga_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", csrc, "-I", os.path.join(ROOT, "include"), str(src),
                           os.path.join(csrc, "cluster_host.cpp"), "-o", str(exe)])
    return str(exe), d


def _selections(words, at, clusters, ks):
    out = {}
    for k in ks:
        eligible, size = int(words[at]), int(words[at + 1])
        selected = [int(c) for c in words[at + 2:at + 2 + size]]
        rank = words[at + 2 + size:at + 2 + size + clusters]
        out[k] = (eligible, selected, rank)
        at += 2 + size + clusters
    assert at == len(words)
    return out


def _run_set(driver, states, w, res, ks):
    exe, d = driver
    n = len(w)
    np.concatenate([np.asarray(states, dtype=np.float64).reshape(n, 4), np.asarray(w, dtype=np.float64).reshape(n, 1)],
                   axis=1).tofile(str(d / "in.bin"))
    subprocess.check_call([exe, "set", str(d / "in.bin"), str(d / "out.bin")] + [repr(float(v)) for v in res] + [str(k) for k in ks])
    words = np.fromfile(str(d / "out.bin"), dtype=np.int64)
    clusters = int(words[0])
    weight = words[1:1 + clusters].view(np.float64)
    count = words[1 + clusters:1 + 2 * clusters]
    return weight, count, _selections(words, 1 + 2 * clusters, clusters, ks)


def _run_pick(driver, weight, count, ks):
    exe, d = driver
    np.stack([np.asarray(weight, dtype=np.float64), np.asarray(count, dtype=np.float64)], axis=1).tofile(str(d / "pick.bin"))
    subprocess.check_call([exe, "pick", str(d / "pick.bin"), str(d / "picked.bin")] + [str(k) for k in ks])
    return _selections(np.fromfile(str(d / "picked.bin"), dtype=np.int64), 0, len(weight), ks)


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


def _bimodal(n):  # the cloud of test_gpu_parity.py::test_cluster_based_estimate_bimodal_cloud_and_update_path
    a = synth.normal_particles(int(n * 0.6), (2.0, 1.0, 0.5), (0.3, 0.3, 0.15), seed=1)
    b = synth.normal_particles(n - len(a), (-4.0, -3.0, -2.0), (0.3, 0.3, 0.15), seed=2)
    states = np.concatenate([a, b])[np.random.Generator(np.random.MT19937(3)).permutation(n)]
    return states, np.random.Generator(np.random.MT19937(4)).gamma(2.0, 1.0, n)


DEFAULTS = (0.2, 0.524, 0.9)
CASES = {
    "multicluster_coarse": (lambda: _multicluster(0.0, 36.0, 0.0, 36.0, 1.0), (1.0, math.pi / 2.0, 0.9)),
    "multicluster_fine": (lambda: _multicluster(-2.0, 2.0, -2.0, 2.0, 0.025), DEFAULTS),
    "bimodal": (lambda: _bimodal(200_000), DEFAULTS),
}
KS = (1, 2, 64)


def _expected_order(weight, count, k):
    eligible = [c for c in range(len(weight)) if count[c] > 1]
    return len(eligible), sorted(eligible, key=lambda c: (-weight[c], c))[:k]


def _check_selection(got, weight, count, k):
    eligible, selected, rank = got
    want_eligible, want = _expected_order(weight, count, k)
    assert eligible == want_eligible
    assert selected == want
    want_rank = np.full(len(weight), -1, dtype=np.int64)
    want_rank[want] = np.arange(len(want))
    assert np.array_equal(rank, want_rank)


@pytest.mark.parametrize("case", sorted(CASES))
def test_cluster_totals_and_selection_on_the_reference_sets(driver, case):
    make, res = CASES[case]
    states, w = make()
    weight, count, picked = _run_set(driver, states, w, res, KS)
    ids = orc.cluster_ids(states, w, *res).astype(np.int64)
    assert len(weight) == ids.max() + 1
    assert np.array_equal(count, np.bincount(ids, minlength=len(weight)))
    # the library adds the cells' sums in cell order, numpy the particles' pairwise: 1e-12 relative, the tolerance of a reported weight
    np.testing.assert_allclose(weight, [w[ids == c].sum() for c in range(len(weight))], rtol=1e-12, atol=0)
    for k in KS:
        _check_selection(picked[k], weight, count, k)
    if case != "bimodal":  # four peaks, the heaviest in the corner where k = 4
        assert picked[64][0] == 4 and len(picked[64][1]) == 4
        assert picked[1][1] == picked[64][1][:1] and picked[2][1] == picked[64][1][:2]
        pose, _ = orc.estimate(states[ids == picked[1][1][0]], w[ids == picked[1][1][0]])
        want_pose, _ = orc.cluster_based_estimate(states, w, *res)
        np.testing.assert_allclose(pose, want_pose, atol=1e-9)  # rank 0 is cluster_based_estimate's cluster


def test_selection_breaks_ties_by_id_and_leaves_single_particles_out(driver):
    #          id:  0    1    2     3    4    5     6    7
    weight = [0.5, 2.0, 0.25, 2.0, 9.0, 0.5, 0.25, 2.0]
    count = [2, 3, 2, 2, 1, 7, 1, 5]  # 4 is the heaviest, and alone; 6 is alone too
    ks = (0, 1, 2, 3, 4, 6, 7, 64)
    picked = _run_pick(driver, weight, count, ks)
    order = [1, 3, 7, 0, 5, 2]
    for k in ks:
        eligible, selected, rank = picked[k]
        assert eligible == 6
        assert selected == order[:k]
        assert rank[4] == -1 and rank[6] == -1
        _check_selection(picked[k], weight, count, k)


def test_selection_of_nothing(driver):
    picked = _run_pick(driver, [0.2, 0.2, 0.2, 0.2], [1, 1, 1, 1], (1, 64))  # NightmareDistributionTest: four singles
    for k in (1, 64):
        assert picked[k][0] == 0 and picked[k][1] == [] and np.all(picked[k][2] == -1)
