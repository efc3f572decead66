"""tests/ndt_reference.py and tests/ndt_families.py held to themselves, without a device: the f64 loop form against the exact form on
every family (keys equal, weights within MEASURED_F64_ERROR, which this file measures), every mutant of the cell choice killed where
the families say it dies, every engineered case shown to reach the threshold it names, and the host layouts (ndt_layout_map,
ndt_layout_map_hashed, compiled from ndt_host.cpp into a program of its own under the address and undefined-behaviour sanitizers)
probed at every centre key and offset the families use against the reference's dictionary look-up."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import ndt_families as fam
import ndt_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def exact(name, number):
    return fam.FAMILIES[name]()[number].exact()


def cases(name):
    return list(enumerate(fam.FAMILIES[name]()))


# ---- the loop form against the exact form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fam.EXACT_FAMILIES)
def test_loop_form_has_the_exact_keys_and_weights_within_the_measured_error(name):
    worst = 0.0
    for number, case in cases(name):
        want, keys, _, _ = exact(name, number)
        got_keys = ref.centre_keys_f64(case.ref_map(), case.states, case.cell_means)
        assert got_keys == keys, case.tag
        got = case.loop()
        assert np.all(np.isfinite(want)) and np.all(want > 0)
        worst = max(worst, float(np.max(np.abs(got - want) / want)))
        vec = case.w0 * ref.weights_vectorized(case.ref_map(), case.states, case.cell_means, case.cell_covs, case.minimum, case.d1, case.d2,
                                               case.kernel) if len(case.cell_means) and not name.startswith(("far", "hashed")) else got
        assert np.max(np.abs(vec - got) / got) <= 4 * 2.0**-53 * (len(case.cell_means) + 4), case.tag  # (numpy's exp against libm's)
    print("ndt f64 loop form against exact, %s: worst relative error %.3g (table %.3g)" % (name, worst, fam.MEASURED_F64_ERROR[name]))
    assert worst <= fam.MEASURED_F64_ERROR[name], "MEASURED_F64_ERROR[%r] is stale: measured %.3g" % (name, worst)
    assert fam.MEASURED_F64_ERROR[name] <= max(4 * worst, 2e-15), "MEASURED_F64_ERROR[%r] is far above what is measured (%.3g)" % (name, worst)


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------------
MUTANT_CASES = 3  # per family: the first, the middle and the last case
KILL = 1e-6
REVEAL = 1e-3  # where a family names the mutant it is for, the wrong cell shows as the revealing maps promise


@functools.lru_cache(maxsize=None)
def kills(name):
    """mutant -> the largest relative change of a weight over the family's sampled cases."""
    all_cases = cases(name)
    sample = sorted({0, len(all_cases) // 2, len(all_cases) - 1})[:MUTANT_CASES]
    out = {}
    for number in sample:
        case = all_cases[number][1]
        want = exact(name, number)[0]
        for mutant, variant in ref.MUTANTS.items():
            got = case.exact(variant)[0]
            out[mutant] = max(out.get(mutant, 0.0), float(np.max(np.abs(got - want) / want)))
    return out


def test_every_mutant_is_killed():
    best = {m: max(kills(name)[m] for name in fam.EXACT_FAMILIES) for m in ref.MUTANTS}
    assert all(v > KILL for v in best.values()), "mutant not killed: %s" % sorted(m for m, v in best.items() if v <= KILL)


@pytest.mark.parametrize("name", fam.WELL_CONDITIONED)
def test_every_cell_choice_family_kills_a_mutant(name):
    assert max(kills(name).values()) > KILL, "mutant not killed: none dies in %s" % name


@pytest.mark.parametrize("name,mutants", [("rotated_edges", ref.FUSED_MUTANTS), ("axis_edges", ("divide_by_resolution",)),
                                          ("box_edges", ref.BOX_MUTANTS), ("hashed_ends", ("wrap_int32",)), ("far_poses", ("wrap_int32",))])
def test_mutants_die_where_the_families_say(name, mutants):
    """(rotated_edges: this is the argument that a translation unit built without -ffp-contract=off fails test_gpu_ndt_edges.py - one
    contraction in ux or uy IS one of the four fused mutants, and each moves a weight of this family by percents.)"""
    for mutant in mutants:
        assert kills(name)[mutant] > REVEAL, "mutant not killed: %s in %s" % (mutant, name)


# ---- each threshold case reaches what it names -----------------------------------------------------------------------------------------------
def test_axis_edges_sit_on_their_edges():
    divide = real = 0
    signs = set()
    for number, case in cases("axis_edges"):
        res, inv = np.float64(case.resolution), np.float64(1.0) / np.float64(case.resolution)
        keys = exact("axis_edges", number)[1]
        for p in case.pairs:
            ux, uy = ref.moved_mean(case.states[p["state"]], case.cell_means[p["cell"]])
            assert (ux, uy) == p["target"], "threshold not reached: %s %s" % (case.tag, p)
            for axis, u in (("x", ux), ("y", uy)):
                if axis not in p["axis"]:
                    continue
                if p["k"] != 0 or p["ulp"] == 0:
                    assert u == fam.edge(p["k"], res, p["ulp"])
                # u is k res (1 + d) with |d| <= 2^-53, a step of one ulp(u) <= 2^-52 |u| away; inv and the product round once more each
                assert abs(u * inv - p["k"]) <= max(5 * np.spacing(np.float64(abs(p["k"]))), 2.0**-50 * case.resolution * 20), (case.tag, p)
                a, b, c = fam.floors_of(u, res)
                assert (a != b) == p["divide"] or not p["divide"]
                divide += int(a != b)
                real += int(a != c)
                signs.add(int(np.sign(keys[p["state"]][p["cell"]][0 if axis == "x" else 1])))
        assert {p["ulp"] for p in case.pairs} == {-1, 0, 1} and {p["axis"] for p in case.pairs} == {"x", "y", "xy"}
        assert {tuple(s[:2]) for s in case.states} == set(fam.QUARTER_TURNS)
        # (weights_exact's own account: every case holds a mean exactly on an edge whose scaled value is the integer itself)
        assert exact("axis_edges", number)[2] == 0.0, "threshold not reached: %s" % case.tag
    assert divide >= 12 and real >= 12, "threshold not reached: floors that differ (%d by division, %d from the real quotient)" % (divide, real)
    assert signs == {-1, 0, 1}
    assert tuple(c.resolution for _, c in cases("axis_edges")) == fam.AXIS_RESOLUTIONS


def test_rotated_edges_flip_under_each_fused_product():
    flips = {m: 0 for m in ref.FUSED_MUTANTS}
    for number, case in cases("rotated_edges"):
        m = case.ref_map()
        keys = exact("rotated_edges", number)[1]
        for p in case.pairs:
            st, mean = case.states[p["state"]], case.cell_means[p["cell"]]
            assert ref.moved_mean(st, mean) == p["target"], "threshold not reached: %s" % (p,)
            plain, fused = ref.centre_key(m, st, mean)[2], ref.centre_key(m, st, mean, ref.MUTANTS[p["flips"]])[2]
            assert plain == keys[p["state"]][p["cell"]] == p["plain"] and fused != plain
            assert abs(st[0]) not in (0.0, 1.0)
            flips[p["flips"]] += 1
        # the nearest any scaled component comes to an integer, by weights_exact's own account: within the rounding of u = k res, of inv
        # and of their product, 2.5 * 2^-52 |k| with |k| <= 6
        assert exact("rotated_edges", number)[2] <= 2.5 * 2.0**-52 * 6, "threshold not reached: %s" % case.tag
    assert min(flips.values()) >= 32, "threshold not reached: %s" % flips


def test_box_edges_stand_where_they_say():
    for number, case in cases("box_edges"):
        m = case.ref_map()
        keys = exact("box_edges", number)[1]
        found_at_reach = []
        for p in case.pairs:
            assert keys[p["state"]][p["cell"]] == p["centre"], "threshold not reached: %s %s" % (case.tag, p)
            found = sum(k is not None for k in ref.neighbours(m, case.kernel, p["centre"]))
            if p["outside"] == case.reach + 1:
                assert found == 0
            if p["outside"] == case.reach:
                found_at_reach.append(found)
        assert {p["outside"] for p in case.pairs} == {case.reach - 1, case.reach, case.reach + 1} and len(case.pairs) == 24
        if len(case.kernel) > 1 or case.kernel != ((0, 0),):
            assert 1 in found_at_reach, "threshold not reached: %s finds %s at reach" % (case.tag, found_at_reach)
    kernels = {c.kernel for _, c in cases("box_edges")}
    assert {ref.DEFAULT_KERNEL, ((0, 0),), fam.REACH_3, fam.REACH_2, fam.ONE_SIDED, fam.FAR_OFFSETS} <= kernels
    assert {len(c.keys) for _, c in cases("box_edges")} >= {1, 2, 6, 25}


def test_far_poses_and_hashed_ends_stand_where_they_say():
    for number, case in cases("far_poses"):
        want, keys, _, _ = exact("far_poses", number)
        floor_only = case.w0 * (1.0 + len(case.cell_means) * case.minimum)
        far = sorted({p["state"] for p in case.pairs})
        assert np.allclose(want[far], floor_only[far], rtol=1e-15) and want[0] > 1.5 * floor_only[0]
        if case.tag == "far_poses[not_finite]":
            assert all(None in cell for i in far for cell in keys[i]) and not np.isfinite(case.states[far]).all(axis=1).any()
            continue
        big = max(abs(k) for i in far for cell in keys[i] for k in cell)
        assert (big <= ref.INT32_MAX) == (case.tag == "far_poses[int32]") and big >= 10**9
    lo, hi = ref.INT32_MIN, ref.INT32_MAX
    for number, case in cases("hashed_ends"):
        keys = exact("hashed_ends", number)[1]
        assert {(lo, lo), (lo + 1, lo), (hi, hi), (hi - 1, hi)} <= {tuple(k) for k in case.keys.tolist()}
        centres = {keys[p["state"]][p["cell"]] for p in case.pairs}
        assert centres == {p["centre"] for p in case.pairs}, "threshold not reached"
        assert (hi + 1, hi) in centres and (lo - 1, lo) in centres and (hi, hi) in centres and (lo, lo) in centres
        assert case.layout == "hashed"


def test_cell_counts_and_conditioning_reach_their_labels():
    assert tuple(len(c.cell_means) for _, c in cases("cell_counts")) == fam.CELL_COUNTS
    for _, case in cases("cell_counts"):
        if len(case.cell_means) < 3:
            continue
        m = case.ref_map()
        terms = [ref.likelihood_at(m, *ref.transform_cell(case.states[0], mean, cov), 0.0, case.d1, case.d2, case.kernel)
                 for mean, cov in zip(case.cell_means, case.cell_covs)]
        assert min(terms) > 0 and max(terms) / min(terms) >= 1e12, "threshold not reached: %s spans %.3g" % (case.tag, max(terms) / min(terms))
    for number, case in cases("conditioning"):
        label = case.pairs[0]["cond"]
        S = ref.transform_cell(case.states[0], case.cell_means[0], case.cell_covs[0])[1] + case.covs[0]
        assert label / 2 <= np.linalg.cond(S) <= label * 2, "threshold not reached: %s" % case.tag
        thin = exact("conditioning", number)[3]  # det / (s00 s11) = 4 / (c + 2 + 1 / c) for these sums: 4 / thin <= 1.21 c from c = 10 on
        assert label / 2 <= (4 / thin if label > 1 else 1 / thin) <= label * 2, "threshold not reached: %s det ratio %.3g" % (case.tag, thin)
    assert tuple(c.pairs[0]["cond"] for _, c in cases("conditioning")) == fam.CONDITIONS


def test_singular_family_holds_every_class_of_term():
    case = fam.singular()[0]
    terms = fam.singular_terms(case)
    assert np.isnan(terms[0, 0]) and np.isnan(terms[0, 1]) and terms[0, 2] == 0.0 and np.isnan(terms[0, 3])  # det == 0 exactly
    assert np.isnan(terms[1, 0])
    assert np.isinf(terms).sum() >= 4 and (terms == 0.0).sum() >= 8 and np.isnan(terms).sum() >= 6, "threshold not reached"
    # the reference's std::max keeps a NaN (its first argument); the loop form does as the reference does
    assert np.isnan(ref.weights(case.ref_map(), case.states[:1], case.cell_means, case.cell_covs, case.minimum, case.d1, case.d2, case.kernel)[0])
    rule = fam.device_rule(case)
    assert np.isfinite(rule[:2]).all() and np.isinf(rule).sum() >= 4 and not np.isnan(rule).any()


def test_revealing_maps_are_well_conditioned_and_reveal_a_wrong_centre():
    """Every map cell well conditioned with its mean inside its own cell; on every case of the well-conditioned families a centre one
    cell off that finds other cells moves the likelihood by more than 1e-3 of it - but for the two `wide` maps (covariances of 2^31
    cells), which show WHETHER a cell was found and not which: there the wrap mutant's effect is held to the same 1e-3
    (test_mutants_die_where_the_families_say)."""
    wide = []
    for name in fam.WELL_CONDITIONED:
        for number, case in cases(name):
            assert max(np.linalg.cond(c) for c in case.covs) < 100
            assert [tuple(k) for k in case.keys.tolist()] == [case.ref_map().cell_near(mean) for mean in case.means]
            if case.wide:
                wide.append(case.tag)
                continue
            pairs = [dict(state=0, cell=j) for j in range(len(case.cell_means))] if name == "far_poses" else None  # (the pose on the map)
            worst = fam.reveals(case, pairs)
            assert 1e-3 < worst < math.inf, (case.tag, worst)
    assert wide == ["far_poses[beyond]", "hashed_ends[wide]"]


# ---- the host layouts, in a program of their own under the sanitizers -----------------------------------------------------------------------------
DRIVER = r"""
// driver <file>: resolution, num_offsets, the offsets, n, n lines "x y", q, q lines "cx cy" (centre keys as the kernels form them).
// Lays the map out both ways and prints, per centre, the record each offset finds: "dense ..." (through the index grid, the kernel's
// index arithmetic) and "hashed ..." (ndt_hash_find_neighbour); a centre outside the centre box prints -2 for every offset.
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "ndt_host.h"

using namespace mcl;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  double resolution;
  mcl_ndt_params prm;
  mcl_default_ndt_params(&prm);
  uint64_t n, q;
  in >> resolution >> prm.num_offsets;
  for (uint32_t k = 0; k < 2 * prm.num_offsets; ++k) in >> prm.offsets[k];
  in >> n;
  std::vector<int32_t> keys(2 * n);
  std::vector<double> means(2 * n, 0.0), covs(4 * n, 0.0);
  for (uint64_t i = 0; i < n; ++i) {
    in >> keys[2 * i] >> keys[2 * i + 1];
    covs[4 * i] = covs[4 * i + 3] = 1.0;
  }
  NdtMapLayout dense;
  NdtHashLayout hashed;
  std::string error;
  const mcl_status ds = ndt_layout_map(keys.data(), means.data(), covs.data(), n, resolution, &prm, &dense, &error);
  const mcl_status hs = ndt_layout_map_hashed(keys.data(), means.data(), covs.data(), n, resolution, &prm, &hashed, &error);
  std::printf("status %d %d grid %" PRId64 " x %" PRId64 "\n", static_cast<int>(ds), static_cast<int>(hs), dense.shape.gw, dense.shape.gh);
  if (hs != MCL_OK) return 1;
  const NdtGridShape g = hashed.shape;
  const NdtHashTable t = hashed.table();
  in >> q;
  for (uint64_t i = 0; i < q; ++i) {
    int64_t cx, cy;
    in >> cx >> cy;
    const bool inside = cx >= g.x0 - g.reach && cx <= g.x1 + g.reach && cy >= g.y0 - g.reach && cy <= g.y1 + g.reach;
    for (int layout = 0; layout < 2; ++layout) {
      if (layout == 0 && ds != MCL_OK) continue;
      std::printf(layout == 0 ? "dense" : "hashed");
      for (uint32_t o = 0; o < prm.num_offsets; ++o) {
        int32_t record = -2;
        if (inside && layout == 0) {
          const int64_t centre = (cy - (g.y0 - g.reach) + g.reach) * g.gw + (cx - (g.x0 - g.reach)) + g.reach;
          record = dense.grid.at(static_cast<size_t>(centre + prm.offsets[2 * o + 1] * g.gw + prm.offsets[2 * o]));
        } else if (inside) {
          record = ndt_hash_find_neighbour(t, cx, cy, prm.offsets[2 * o], prm.offsets[2 * o + 1]);
        }
        std::printf(" %d", record);
      }
      std::printf("\n");
    }
  }
  return 0;
}
"""


def test_host_layouts_find_the_dictionarys_cells_under_the_sanitizers(tmp_path):
    """One stand-alone program (its own main, ndt_host.cpp compiled with it, -fsanitize=address,undefined) lays out the map of every case
    of every family but singular - box_edges' far-offsets map has the largest border the index grid can have, 128 cells a side - and
    probes both layouts at every centre key the family's (state, cell) pairs reach, and one cell around each, with every offset: the
    record found is the one the reference's dictionary look-up finds."""
    src = tmp_path / "driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "ndt_layout_san"
    csrc = os.path.join(ROOT, "beluga_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc, "-I", os.path.join(ROOT, "include"), str(src),
                           os.path.join(csrc, "ndt_host.cpp"), "-o", str(exe)])
    probed = 0
    for name in fam.EXACT_FAMILIES:
        for number, case in cases(name):
            m = case.ref_map()
            number_of = {tuple(k): i for i, k in enumerate(case.keys.tolist())}
            # (centres the driver can read: a component that is not finite has no key, and one beyond int64 - far_poses from 1e100 on -
            # cannot be written as the kernels' 64-bit centre either; the kernels' box test turns both away in f64)
            centres = sorted({(c[0] + dx, c[1] + dy) for row in exact(name, number)[1] for c in row for dx in (-1, 0, 1) for dy in (-1, 0, 1)
                              if None not in c and max(abs(c[0]), abs(c[1])) < 2**62})
            lines = [repr(case.resolution), str(len(case.kernel)), " ".join("%d %d" % o for o in case.kernel), str(len(case.keys))]
            lines += ["%d %d" % tuple(k) for k in case.keys.tolist()] + [str(len(centres))] + ["%d %d" % c for c in centres]
            path = tmp_path / "in.txt"
            path.write_text("\n".join(lines) + "\n")
            done = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
            assert done.returncode == 0 and "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr, (case.tag, done.stderr)
            out = done.stdout.splitlines()
            dense_ok = out[0].split()[1] == "0"
            assert dense_ok == (case.layout == "both"), out[0]
            if case.tag == "box_edges[far_offsets]":
                assert out[0].endswith("grid 321 x 257")
            rows = out[1:]
            per = 2 if dense_ok else 1
            assert len(rows) == per * len(centres)
            for i, centre in enumerate(centres):
                want = [number_of[k] if k is not None else -1 for k in ref.neighbours(m, case.kernel, centre)]
                for row in rows[per * i:per * i + per]:
                    got = [int(v) for v in row.split()[1:]]
                    if got[0] == -2:  # outside the centre box: the kernels look nothing up, and the dictionary holds nothing there
                        assert want == [-1] * len(case.kernel), (case.tag, centre)
                    else:
                        assert got == want, (case.tag, centre, row)
                    probed += 1
    assert probed > 5000
