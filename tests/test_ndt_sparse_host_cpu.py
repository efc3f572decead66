"""The hashed layout of the NDT map (mcl_set_ndt_map_layout) on the CPU, in the manner of test_ndt_small_host_cpu.py: a plain g++
compiles ndt_host.cpp with a short driver that reads a map and queries from a file, lays the map out both ways (ndt_layout_map,
ndt_layout_map_hashed) and prints the statuses, the table and what ndt_hash_find / ndt_hash_find_neighbour - the functions the kernels
call - return.  The hash, the capacity rule and the longest probe are restated here (ndt_sparse_cases.py) from the words of ndt_hash.h;
the same driver runs once more over the same inputs under the address and undefined-behaviour sanitizers, as a program of its own."""
import os
import re
import subprocess

import numpy as np
import pytest

import ndt_sparse_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -7

DRIVER = r"""
// driver <file>: resolution, n, then n lines "x y mx my c00 c01 c10 c11"; q, then q lines "x y" (ndt_hash_find);
//                b, then b lines "cx cy dx dy" (ndt_hash_find_neighbour).  Reals as strtod reads them (hex floats, nan, inf).
// prints: "fits <ndt_keys_fit_grid>", "dense <status> <message>", "hashed <status> <message>", and where the hashed layout was built "table <log2> <longest>",
//         "slot <index> <key> <record>" per occupied slot, "records <1 if they equal the dense layout's or that one was refused>",
//         "shape <reach> <x0> <y0> <x1> <y1> <fits>", "find <record>" per query, "near <record>" per neighbour query.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "ndt_host.h"

using namespace mcl;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string word;
  auto real = [&] { in >> word; return std::strtod(word.c_str(), nullptr); };
  auto whole = [&] { in >> word; return std::strtoll(word.c_str(), nullptr, 0); };
  const double resolution = real();
  const uint64_t n = static_cast<uint64_t>(whole());
  std::vector<int32_t> keys(2 * n);
  std::vector<double> means(2 * n), covs(4 * n);
  for (uint64_t i = 0; i < n; ++i) {
    keys[2 * i] = static_cast<int32_t>(whole());
    keys[2 * i + 1] = static_cast<int32_t>(whole());
    for (int k = 0; k < 2; ++k) means[2 * i + k] = real();
    for (int k = 0; k < 4; ++k) covs[4 * i + k] = real();
  }
  NdtMapLayout dense;
  NdtHashLayout hashed;
  std::string dense_error, hashed_error;
  const mcl_status ds = ndt_layout_map(keys.data(), means.data(), covs.data(), n, resolution, nullptr, &dense, &dense_error);
  const mcl_status hs = ndt_layout_map_hashed(keys.data(), means.data(), covs.data(), n, resolution, nullptr, &hashed, &hashed_error);
  std::printf("fits %d\n", ndt_keys_fit_grid(keys.data(), n, nullptr) ? 1 : 0);
  std::printf("dense %d %s\n", static_cast<int>(ds), dense_error.c_str());
  std::printf("hashed %d %s\n", static_cast<int>(hs), hashed_error.c_str());
  if (hs != MCL_OK) return 0;
  std::printf("table %u %u\n", hashed.log2_capacity, hashed.longest_probe);
  for (size_t s = 0; s < hashed.slots.size(); ++s)
    if (hashed.slots[s].record >= 0) std::printf("slot %zu %" PRIu64 " %d\n", s, hashed.slots[s].key, hashed.slots[s].record);
  std::printf("records %d\n", ds != MCL_OK || dense.records == hashed.records ? 1 : 0);
  const NdtGridShape& g = hashed.shape;
  std::printf("shape %d %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d\n", g.reach, g.x0, g.y0, g.x1, g.y1, g.fits ? 1 : 0);
  const NdtHashTable t = hashed.table();
  const long long q = whole();
  for (long long i = 0; i < q; ++i) {
    const int32_t x = static_cast<int32_t>(whole()), y = static_cast<int32_t>(whole());
    std::printf("find %d\n", ndt_hash_find(t, ndt_pack_key(x, y)));
  }
  const long long b = whole();
  for (long long i = 0; i < b; ++i) {
    const int64_t cx = whole(), cy = whole();
    const int32_t dx = static_cast<int32_t>(whole()), dy = static_cast<int32_t>(whole());
    std::printf("near %d\n", ndt_hash_find_neighbour(t, cx, cy, dx, dy));
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
                          ["-I", csrc, "-I", os.path.join(ROOT, "include"), str(src), os.path.join(csrc, "ndt_host.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("ndt_sparse_host"), "driver", [])


def _real(v):
    return float(v).hex() if np.isfinite(v) else repr(float(v))


def write_input(path, keys, resolution=1.0, means=None, covs=None, finds=(), nears=()):
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 2)
    if means is None:
        means, covs = cases.cells_for(keys, resolution if np.isfinite(resolution) and resolution > 0 else 1.0)
    lines = [_real(resolution), str(len(keys))]
    for k, m, c in zip(keys, np.asarray(means).reshape(-1, 2), np.asarray(covs).reshape(-1, 4)):
        lines.append(" ".join([str(int(k[0])), str(int(k[1]))] + [_real(v) for v in m] + [_real(v) for v in c]))
    lines.append(str(len(finds)))
    lines += [f"{int(x)} {int(y)}" for x, y in finds]
    lines.append(str(len(nears)))
    lines += [" ".join(str(int(v)) for v in row) for row in nears]
    path.write_text("\n".join(lines) + "\n")
    return str(path)


class Result:
    def __init__(self, text):
        self.slots, self.find, self.near, self.table, self.records, self.shape = {}, [], [], None, None, None
        for line in text.splitlines():
            head, _, rest = line.partition(" ")
            if head in ("dense", "hashed"):
                status, _, message = rest.partition(" ")
                setattr(self, head, (int(status), message))
            elif head == "fits":
                self.fits = int(rest)
            elif head == "table":
                self.table = tuple(int(w) for w in rest.split())
            elif head == "slot":
                s, key, record = (int(w) for w in rest.split())
                self.slots[s] = (key, record)
            elif head == "records":
                self.records = int(rest)
            elif head == "shape":
                self.shape = tuple(int(w) for w in rest.split())
            elif head == "find":
                self.find.append(int(rest))
            elif head == "near":
                self.near.append(int(rest))


def run(exe, path):
    return Result(subprocess.check_output([exe, path], text=True))


def check_table(keys, r):
    """Capacity a power of two with load <= 1/2, every key in one slot with its record number, every slot between a key's home and
    its own occupied, and the recorded longest probe the true one."""
    keys = np.asarray(keys).reshape(-1, 2)
    log2, longest = r.table
    assert log2 == cases.log2_capacity(len(keys)) and 2 * len(keys) <= (1 << log2)
    assert log2 == 1 or (1 << (log2 - 1)) < 2 * len(keys)  # (the smallest such power)
    capacity = 1 << log2
    assert len(r.slots) == len(keys) and all(0 <= s < capacity for s in r.slots)
    want = {cases.pack(x, y): i for i, (x, y) in enumerate(keys)}
    assert {key: record for key, record in r.slots.values()} == want
    true_longest = 1
    for s, (key, _) in r.slots.items():
        h = ((key * cases.MULTIPLIER) & (2**64 - 1)) >> (64 - log2)
        distance = (s - h) % capacity
        assert all(((h + d) % capacity) in r.slots for d in range(distance))
        true_longest = max(true_longest, distance + 1)
    assert longest == true_longest
    return true_longest


# ---- found and not found; the table's shape ---------------------------------------------------------------------------------------------
def absent_queries(keys):
    """Keys the map does not hold: every neighbour of a stored key, keys 1 and 2^20 away, and keys whose home slot another key has."""
    stored = {(int(x), int(y)) for x, y in keys}
    out = set()
    for x, y in stored:
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                out.add((x + dx, y + dy))
        for step in (1, 2**20):
            out.update({(x + step, y), (x - step, y), (x, y + step), (x, y - step)})
    c = cases.log2_capacity(len(stored))
    homes = {cases.home(x, y, c) for x, y in stored}
    taken = [(x, y) for x in range(1000, 1400) for y in (3, -900) if cases.home(x, y, c) in homes]
    assert len(taken) >= 50
    out.update(taken)
    return sorted(out - stored), taken


def test_every_stored_key_is_found_and_no_other(driver, tmp_path):
    keys = cases.holes_keys()
    assert 200 <= len(keys) <= 400
    absent, taken = absent_queries(keys)
    r = run(driver, write_input(tmp_path / "holes.txt", keys, 0.5, finds=[tuple(k) for k in keys] + absent))
    assert r.dense[0] == OK and r.hashed == (OK, "") and r.records == 1 and r.fits == 1
    assert r.find[:len(keys)] == list(range(len(keys)))
    assert r.find[len(keys):] == [-1] * len(absent)
    longest = check_table(keys, r)
    assert longest >= 2  # (the map does exercise the probe beyond the home slot)
    assert r.shape == (1, int(keys[:, 0].min()), int(keys[:, 1].min()), int(keys[:, 0].max()), int(keys[:, 1].max()), 1)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 31, 32, 33, 64, 1000])
def test_table_shape_at_the_edges_of_the_capacity_rule(driver, tmp_path, n):
    rng = np.random.Generator(np.random.PCG64(n))
    keys = np.unique(rng.integers(-500, 500, (3 * n, 2)), axis=0)
    rng.shuffle(keys)
    keys = keys[:n]
    r = run(driver, write_input(tmp_path / "shape.txt", keys, finds=[tuple(k) for k in keys]))
    assert r.hashed == (OK, "") and r.find == list(range(n))
    check_table(keys, r)
    assert r.table[0] == {1: 1, 2: 2, 3: 3, 4: 3, 5: 4, 31: 6, 32: 6, 33: 7, 64: 7, 1000: 11}[n]


# ---- collisions --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [8, 12])
def test_keys_that_share_one_home_slot_all_resolve(driver, tmp_path, count):
    keys = cases.colliding_keys(count)
    c = cases.log2_capacity(count)
    assert len(keys) == count and len({cases.home(x, y, c) for x, y in keys}) == 1
    absent = [(int(x), int(y) + 1) for x, y in keys] + [(int(keys[-1][0]) + 1 + i, int(keys[0][1])) for i in range(40)]
    absent = [k for k in absent if k not in {tuple(map(int, k2)) for k2 in keys}]
    r = run(driver, write_input(tmp_path / "collide.txt", keys, finds=[tuple(k) for k in keys] + absent))
    assert r.hashed == (OK, "") and r.find == list(range(count)) + [-1] * len(absent)
    assert check_table(keys, r) == count  # (the last of them sits count - 1 slots behind the home they share)
    h = cases.home(*keys[0], c)
    assert sorted(r.slots) == sorted((h + d) % (1 << c) for d in range(count))


# ---- keys of both signs and at the ends of the int32 range -----------------------------------------------------------------------------------
def extreme_keys():
    lo, hi = cases.INT32_MIN, cases.INT32_MAX
    return np.array([(hi, hi), (-hi, -hi), (hi, -hi), (-hi, hi), (lo, lo), (lo, hi), (hi, lo), (0, 0), (-1, -1), (-1, 0), (0, -1), (5, lo), (lo, 5),
                     (-2_000_000_000, 2_000_000_000), (2_000_000_000, -2_000_000_000)], dtype=np.int64)


def test_extreme_keys_and_neighbours_beyond_int32(driver, tmp_path):
    keys = extreme_keys()
    lo, hi = cases.INT32_MIN, cases.INT32_MAX
    absent = [(hi - 1, hi), (lo + 1, lo), (1, 1), (-2, -1), (hi, 0), (0, lo)]
    # neighbour queries: (centre, offset, the stored key's number or -1).  A neighbour beyond int32 is not probed although the key it
    # would wrap onto IS stored: (hi, hi) + (1, 0) wraps onto (lo, hi), (5, lo) - (0, 1) onto (5, hi) ... (lo, hi) and (hi, lo) are there.
    number = {tuple(map(int, k)): i for i, k in enumerate(keys)}
    nears = [((hi, hi, 0, 0), number[(hi, hi)]), ((hi, hi, 1, 0), -1), ((hi, hi, 0, 1), -1), ((hi, hi, 1, 1), -1),
             ((lo, lo, 0, 0), number[(lo, lo)]), ((lo, lo, -1, 0), -1), ((lo, lo, 0, -1), -1), ((lo, hi, -1, 0), -1), ((hi, lo, 0, -1), -1),
             ((lo, hi, 0, 1), -1), ((hi, lo, 1, 0), -1),
             # a centre that is itself beyond int32 (the centre box has a border of `reach`) still finds the neighbour inside
             ((hi + 1, hi, -1, 0), number[(hi, hi)]), ((hi + 1, hi + 1, -1, -1), number[(hi, hi)]), ((lo - 1, lo - 1, 1, 1), number[(lo, lo)]),
             ((hi + 1, hi, 0, 0), -1), ((lo - 1, 5, 0, 0), -1), ((lo - 64, 5, 64, 0), number[(lo, 5)]), ((hi + 64, lo, -64, 0), number[(hi, lo)]),
             ((0, 0, -1, -1), number[(-1, -1)]), ((0, 0, -1, 0), number[(-1, 0)]), ((-1, -1, 1, 1), number[(0, 0)]), ((0, 0, 1, 1), -1)]
    r = run(driver, write_input(tmp_path / "extreme.txt", keys, finds=[tuple(k) for k in keys] + absent, nears=[q for q, _ in nears]))
    assert r.dense[0] == UNSUPPORTED and "exceeds 2^26 cells" in r.dense[1] and r.fits == 0  # (asked first, the same answer)
    assert r.hashed == (OK, "")
    assert r.find == list(range(len(keys))) + [-1] * len(absent)
    assert r.near == [want for _, want in nears]
    check_table(keys, r)
    assert r.shape == (1, lo, lo, hi, hi, 0)


# ---- refusals: ndt_layout_map's, status and words --------------------------------------------------------------------------------------------
def _refusals():
    keys = np.array([(0, 0), (3, -2), (-4, 1), (3, -2), (7, 7)])
    means, covs = cases.cells_for(keys, 1.0)
    out = {"duplicate": dict(keys=keys, want="duplicate key (3, -2)"), "no_cells": dict(keys=keys[:0], want="no cells")}
    fine = np.delete(keys, 3, axis=0)
    fm, fc = np.delete(means, 3, axis=0), np.delete(covs, 3, axis=0)
    for name, resolution in (("resolution_zero", 0.0), ("resolution_negative", -1.0), ("resolution_nan", float("nan")),
                             ("resolution_infinite", float("inf"))):
        out[name] = dict(keys=fine, resolution=resolution, want="resolution must be positive and finite")
    for name, (row, col, value) in {"mean_nan": (1, 0, float("nan")), "mean_infinite": (2, 1, float("inf"))}.items():
        m = fm.copy()
        m[row, col] = value
        out[name] = dict(keys=fine, means=m, covs=fc, want=f"cell {row} has a value that is not finite")
    c = fc.copy()
    c[3, 1, 1] = float("-inf")
    out["covariance_infinite"] = dict(keys=fine, means=fm, covs=c, want="cell 3 has a value that is not finite")
    c = fc.copy()
    c[0, 0, 1] += 1e-3
    out["covariance_asymmetric"] = dict(keys=fine, means=fm, covs=c, want="the covariance of cell 0 is not symmetric")
    # (the order of the checks: a value that is not finite is reported before a duplicate that comes earlier in the list)
    m = means.copy()
    m[4, 0] = float("nan")
    out["not_finite_before_duplicate"] = dict(keys=keys, means=m, covs=covs, want="cell 4 has a value that is not finite")
    return out


REFUSALS = _refusals()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_are_the_dense_layouts(driver, tmp_path, name):
    case = dict(REFUSALS[name])
    want = case.pop("want")
    r = run(driver, write_input(tmp_path / "refused.txt", case.pop("keys"), case.pop("resolution", 1.0), **case))
    assert r.dense[0] == INVALID and want in r.dense[1] and r.dense[1].startswith("mcl_set_ndt_map: ")
    assert r.hashed == r.dense
    assert r.table is None and r.fits == 1  # (what is refused anyway counts as fitting: the dense layout's words are reported)


# ---- the same driver under the sanitizers, as a program of its own ------------------------------------------------------------------------------
def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = _compile(tmp_path, "driver_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    holes = cases.holes_keys()
    absent, _ = absent_queries(holes)
    hi, lo = cases.INT32_MAX, cases.INT32_MIN
    inputs = [write_input(tmp_path / "a.txt", holes, 0.5, finds=[tuple(k) for k in holes] + absent),
              write_input(tmp_path / "b.txt", cases.colliding_keys(12), finds=[tuple(k) for k in cases.colliding_keys(12)]),
              write_input(tmp_path / "c.txt", extreme_keys(), finds=[tuple(k) for k in extreme_keys()],
                          nears=[(hi, hi, 1, 1), (lo, lo, -1, -1), (hi + 64, lo, -64, 0), (lo - 64, 5, 64, 0), (hi + 1, hi + 1, 0, 0)]),
              write_input(tmp_path / "d.txt", np.array([(0, 0)]), finds=[(0, 0), (1, 0), (-1, -1)], nears=[(0, 0, 0, 0)])]
    for i, name in enumerate(sorted(REFUSALS)):
        case = dict(REFUSALS[name])
        case.pop("want")
        inputs.append(write_input(tmp_path / f"r{i}.txt", case.pop("keys"), case.pop("resolution", 1.0), **case))
    for path in inputs:
        done = subprocess.run([exe, path], capture_output=True, text=True)
        assert done.returncode == 0 and "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr, (path, done.stderr)
        assert done.stdout.startswith("fits ")


# ---- header and bindings ------------------------------------------------------------------------------------------------------------------------
def test_header_and_bindings_name_the_calls():
    from beluga_amd import capi
    text = open(os.path.join(ROOT, "include", "beluga_mcl.h")).read()
    for word in ("mcl_set_ndt_map_layout", "mcl_get_ndt_map_layout"):
        assert re.search(r"\b" + word + r"\b", text), word
        assert word in capi.exported_names()
    assert capi._SIGNATURES["mcl_set_ndt_map_layout"][1] == [capi._ctx, capi.C.c_int32]
    assert len(capi._SIGNATURES["mcl_get_ndt_map_layout"][1]) == 3
