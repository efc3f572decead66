"""tests/landmark_reference.py and tests/landmark_families.py held to themselves, without a device: the exact form against the numpy
restatement on the reference's own cases (LANDMARK_CASES and BEARING_CASES of test_landmark_cpu.py, with their closed forms) and on a
scattered scene of this file's own, the f64 loop form (lane and wave walks) against the exact form on every family
(picks equal, weights within MEASURED_F64_ERROR, which this file measures), every mutant killed in the family that is there for it,
every engineered case shown to reach what it names, and the host plumbing (landmark_layout_map, landmark_records: compiled from
landmark_host.cpp into a program of its own under the address and undefined-behaviour sanitizers) against the restated plumbing."""
import functools
import math
import os
import subprocess

import mpmath
import numpy as np
import pytest

import landmark_families as fam
import landmark_reference as ref
from test_landmark_cpu import BEARING, BEARING_CASES, BOX, LANDMARK, LANDMARK_CASES, POSE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KILL = 1e-6
REVEAL = 1e-3


@functools.lru_cache(maxsize=None)
def exact(name, number):
    return fam.FAMILIES[name]()[number].exact()


def cases(name):
    return list(enumerate(fam.FAMILIES[name]()))


# ---- the exact form against the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,name", [("landmark", n) for n in sorted(LANDMARK_CASES)] + [("bearing", n) for n in sorted(BEARING_CASES)])
def test_exact_form_on_the_reference_cases(model, name):
    """weights_exact at the reference tests' pose on each of their cases, a prior weight of 1: within the reference's own tolerance of its
    expectation; equal to the closed form the case stands for (1 + P, exp(-1/2) + P, P for the empty map and for a category the map does
    not have, 0 for those in the bearing model) and to the restatement within 1e-12, the bound the restatement itself is held to on
    these cases (POSE's cosine is cos(-pi/2) in f64, 6e-17 and not 0, and the exact form takes it as given); and the loop form picks
    the same landmarks and stays within the same bound."""
    bearing = model == "bearing"
    entries, detections, expected, tolerance, closed = (BEARING_CASES if bearing else LANDMARK_CASES)[name]
    lmap = ref.LandmarkMap([e[0] for e in entries], [e[1] for e in entries], BOX)
    det, dcat = [d[0] for d in detections], [d[1] for d in detections]
    params = BEARING if bearing else LANDMARK
    want, picks = ref.weights_exact(lmap, POSE, det, dcat, [1.0], bearing, **params)
    assert len(want) == 1 and abs(float(want[0]) - expected) <= tolerance
    if closed is not None:
        assert float(want[0]) == pytest.approx(closed, rel=1e-12, abs=0.0)
        assert (want[0] == 0) == (closed == 0.0)
    restated = (ref.bearing_weights if bearing else ref.landmark_weights)(lmap, POSE, det, dcat, **params)[0]
    assert ref.excess_errors(restated, want).max() <= 1e-12
    for wave in (False, True):
        loop, loop_picks, _ = ref.weights_loop(lmap, POSE, det, dcat, [1.0], bearing, wave=wave, **params)
        assert loop_picks == picks and ref.excess_errors(loop, want).max() <= 1e-12
    has = {int(c) for c in lmap.categories}
    assert picks == [[0 if c in has else None for c in dcat]]  # (no category of these maps has two landmarks)


@pytest.mark.parametrize("bearing", [False, True], ids=["landmark", "bearing"])
def test_exact_form_agrees_with_the_restatement(bearing):
    """Beside the reference's cases, whose categories hold one landmark each, a scene with a search in it.  A scattered scene of six categories (the sizes of test_gpu_landmark_small.py's), 40 poses, 9 detections with a category the map does
    not have in the landmark model: the restatement (numpy, the kernel's order) stands within the f64 cost of its own operations of the
    exact form - 1e-12, the bound its tests have used - and the loop form returns the restatement's weights up to numpy's functions."""
    rng = np.random.Generator(np.random.PCG64(2))
    sizes = {10: 1, 11: 2, 12: 63, 13: 64, 14: 65, 15: 130}
    cat = rng.permutation(np.concatenate([np.full(c, k) for k, c in sizes.items()])).astype(np.uint32)
    pos = np.column_stack([rng.uniform(-12.0, 12.0, (len(cat), 2)), rng.uniform(0.0, 2.0, len(cat))])
    lmap = ref.LandmarkMap(pos, cat)
    states = np.array([fam.pose(rng.uniform(-3, 3), rng.uniform(-6, 6), rng.uniform(-6, 6)) for _ in range(40)])
    det = np.column_stack([rng.uniform(-8.0, 8.0, (9, 2)), rng.uniform(-0.5, 1.5, 9)])
    dcat = np.array([10, 11, 12, 13, 14, 15, 12, 15, 15 if bearing else 99], dtype=np.uint32)
    w0 = fam._w0(40, 1)
    if bearing:
        params = dict(sigma_bearing=0.3, sensor_pose_in_robot=fam.TILTED)
        restated, gaps = ref.bearing_weights(lmap, states, det, dcat, **params)
    else:
        params = dict(sigma_range=0.8, sigma_bearing=0.3, random_prob=1e-4)
        restated, gaps = ref.landmark_weights(lmap, states, det, dcat, **params)
    assert gaps.min() > 1e-9
    want, picks = ref.weights_exact(lmap, states, det, dcat, w0, bearing, **params)
    for wave in (False, True):
        loop, loop_picks, exponents = ref.weights_loop(lmap, states, det, dcat, w0, bearing, wave=wave, **params)
        assert loop_picks == picks
        # (numpy's sqrt, arctan2 and exp against libm's: the reasoning of landmark_families.rule_bound)
        assert np.all(np.abs(loop - w0 * restated) / loop <= (12.0 * exponents + 3 * 9 + 1) * 2.0**-53)
    assert ref.excess_errors(w0 * restated, want).max() <= 1e-12


# ---- the loop form against the exact form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fam.FAMILIES))
def test_loop_form_has_the_exact_picks_and_weights_within_the_measured_error(name):
    worst = 0.0
    for number, case in cases(name):
        want, picks = exact(name, number)
        lane = case.loop()
        wave = case.loop(wave=True)
        assert lane[1] == picks and wave[1] == picks, case.tag
        assert np.array_equal(lane[0].view(np.uint64), wave[0].view(np.uint64)), case.tag
        assert not np.isnan(lane[0]).any() and not np.signbit(lane[0]).any(), case.tag
        worst = max(worst, float(ref.excess_errors(lane[0], want, case.absolute_steps()).max()))
    print("landmark f64 loop form against exact, %s: worst relative error %.3g (table %.3g)" % (name, worst, fam.MEASURED_F64_ERROR[name]))
    assert worst <= fam.MEASURED_F64_ERROR[name], "MEASURED_F64_ERROR[%r] is stale: measured %.3g" % (name, worst)
    assert fam.MEASURED_F64_ERROR[name] <= max(4 * worst, 2e-15), "MEASURED_F64_ERROR[%r] is far above what is measured (%.3g)" % (name, worst)


@pytest.mark.parametrize("name", sorted(fam.RULE_FAMILIES))
def test_rule_families_walk_the_same_in_both_forms(name):
    for case in fam.RULE_FAMILIES[name]():
        lane, wave = case.loop()[0], case.loop(wave=True)[0]
        assert np.array_equal(np.isnan(lane), np.isnan(wave)) and np.array_equal(lane[~np.isnan(lane)], wave[~np.isnan(wave)]), case.tag
        assert not np.signbit(lane[~np.isnan(lane)]).any()


def test_rule_families_hold_the_classes_their_docstring_names():
    for case in fam.not_finite_poses():
        got = case.loop()[0]
        broken = ~np.isfinite(case.states).all(axis=1)
        has_landmark = any(int(c) in (1, 2, 3) for c in case.dcat)
        assert broken.sum() == 9 and np.array_equal(np.isnan(got), broken & has_landmark), case.tag
        huge = np.flatnonzero(np.abs(case.states[:, 2:]).max(axis=1) == 1e300)
        assert len(huge) == 3
        if has_landmark and not case.bearing:  # every term with a landmark is random_prob (+ 0)
            np.testing.assert_allclose(got[huge], case.w0[huge] * case.params["random_prob"] ** case.k, rtol=1e-14)
        if has_landmark and case.bearing:  # every term is exp(0) or exp(-pi^2 / den), by the sign of the zero dot product
            low = math.exp(-math.pi**2 / (2 * case.params["sigma_bearing"] ** 2))
            ratio = np.log(got[huge] / case.w0[huge]) / math.log(low)
            assert np.allclose(ratio, np.rint(ratio), atol=1e-9) and np.all(ratio > -1e-9) and np.all(ratio < case.k + 1e-9), ratio
    landmark, bearing = fam.overflow_underflow()
    got = landmark.loop()[0]
    assert np.all(np.isfinite(got)) and np.all(got > 0)
    # the 1e150 detections' terms are random_prob exactly: the weight is at least w0 rp^3 times the other three terms' floor rp^3
    assert np.all(got >= landmark.w0 * landmark.params["random_prob"] ** 6)
    got = bearing.loop()[0]
    assert np.all(np.isfinite(got)) and np.all(got > 0)


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def killed_in(mutant):
    """The cases of the mutant's own family on which it moves a weight by more than KILL of it."""
    name = fam.MUTANT_DIES_IN[mutant]
    out = []
    for number, case in cases(name):
        want = exact(name, number)[0]
        got = case.loop(variant=ref.MUTANTS[mutant], wave=mutant in fam.WAVE_ONLY)[0]
        if ref.excess_errors(got, want, case.absolute_steps()).max() > KILL:
            out.append(case.tag)
    return out


def test_the_table_names_every_mutant():
    assert set(fam.MUTANT_DIES_IN) == set(ref.MUTANTS) == set(fam.MUTANT_DIES_ON) and len(ref.MUTANTS) == 12
    assert all(len(tags) >= 1 for tags in fam.MUTANT_DIES_ON.values())


@pytest.mark.parametrize("mutant", sorted(ref.MUTANTS))
def test_every_mutant_dies_where_the_table_says(mutant):
    """In its family, and there on every case that MUTANT_DIES_ON names for it."""
    dead = killed_in(mutant)
    print("landmark mutant %s dies on %d cases of %s, first %s" % (mutant, len(dead), fam.MUTANT_DIES_IN[mutant], dead[:1]))
    assert dead, "mutant not killed: %s in %s" % (mutant, fam.MUTANT_DIES_IN[mutant])
    tags = {case.tag for _, case in cases(fam.MUTANT_DIES_IN[mutant])}
    for tag in fam.MUTANT_DIES_ON[mutant]:
        assert tag in tags, "no such case: %s" % tag
        assert tag in dead, "mutant not killed: %s on %s" % (mutant, tag)


def test_mutants_die_on_the_cases_built_for_them():
    """The strided scan's last partial stride is met at placement (5, 129) with g = 64; a tie between lanes needs g > 1; a lane without
    a candidate needs a category smaller than g; the bearing plumbing dies in bearing cases only."""
    assert any("at=(5, 129)" in tag and "k=1," in tag for tag in killed_in("drop_last_stride"))
    assert all("k=33" not in tag for tag in killed_in("wave_tie_to_larger")) and all("equal" in tag for tag in killed_in("wave_tie_to_larger"))
    assert all("equal" in tag for tag in killed_in("last_of_equals"))
    assert {tag.split(",")[1] for tag in killed_in("fma_d2")} >= {"origin", "utm"}
    assert all("bearing" in tag for tag in killed_in("bearing_slot_collides") + killed_in("bearing_run_shared"))
    assert any("absent" in tag for tag in killed_in("count0_as_1")) and any("landmark" in tag for tag in killed_in("count0_as_1"))
    for mutant in ("range_first_minus_1", "range_count_plus_1"):
        assert any("landmark" in tag for tag in killed_in(mutant)) and any("bearing" in tag for tag in killed_in(mutant))


# ---- each engineered case reaches what it names ------------------------------------------------------------------------------------------------
def test_near_ties_meet_their_class_and_the_pick_decides():
    kinds = {offset: set() for offset in fam.TIE_OFFSETS}
    combos = set()
    for number, case in cases("near_ties"):
        m = case.meta
        p, a, b = m["point"], m["along"], m["across"]
        assert p == ref.world_point(tuple(case.states[0]), tuple(case.det[0]))
        assert fam.tie_kind(a, b, p) == m["kind"], "threshold not reached: %s" % case.tag
        fa, fb = fam.d2_f64(a, p), fam.d2_f64(b, p)
        assert abs(fa - fb) <= np.spacing(min(fa, fb)) and fam.d2_exact(a, p) != fam.d2_exact(b, p)
        grouped = ref.layout(case.ref_map())[0]
        assert {tuple(grouped[m["at"][0]]), tuple(grouped[m["at"][1]])} == {a, b} and len(grouped) == 130
        others = [fam.d2_f64(l, p) for i, l in enumerate(grouped) if i not in m["at"]]
        assert min(others) > 1e5 * fa
        # picking the other one moves the term by more than 1e-3 of it: one detection against a map of A alone and of B alone
        terms = [ref.weights_exact(ref.LandmarkMap([l], [7]), case.states[:1], case.det[:1], [7], [1.0], **case.params)[0][0] for l in (a, b)]
        assert abs(terms[0] - terms[1]) > REVEAL * max(terms), "threshold not reached: %s" % case.tag
        pick = exact("near_ties", number)[1][0][0]
        assert pick in m["at"] and all(row == [pick] * case.k for row in exact("near_ties", number)[1])
        kinds[m["offset"]].add(m["kind"])
        combos.add((m["pose"], m["offset"], m["kind"], m["order"]))
        assert tuple(grouped[m["at"][m["order"]]]) == a  # order 0: A first in map order
    assert all(found == set(fam.TIE_KINDS) for found in kinds.values()), "threshold not reached: %s" % kinds
    assert len(combos) == 36  # every pose x offset x kind in both orders
    assert {c.k for _, c in cases("near_ties")} == set(fam.TIE_KS)
    for k in fam.TIE_KS:
        assert {c.meta["at"] for _, c in cases("near_ties") if c.k == k} == set(fam.tie_placements(k))


def test_range_leaks_bait_both_ends_of_every_range():
    for bearing, params in ((False, fam.LEAK_PARAMS), (True, fam.LEAK_BEARING)):
        pos, cat = fam.leak_map(bearing, params)
        lmap = ref.LandmarkMap(pos, cat)
        grouped, cats, ranges = ref.layout(lmap)
        assert {c: n for c, (_, n) in ranges.items()} == fam.LEAK_SIZES and sorted(ranges) == [0, 1, 7, 8, 9, 0xFFFFFFFE, 0xFFFFFFFF]
        assert len(set(np.flatnonzero(np.diff(cat.astype(np.int64)) != 0))) > 100  # interleaved in map order
        state = fam._leak_states(3)[0]
        present = sorted(ranges)
        for n, c in enumerate(present):
            first, count = ranges[c]
            point = np.array(fam._bait_point(state, fam._leak_vector(c, bearing), bearing, params))
            if n > 0:
                assert np.array_equal(grouped[first - 1], point), (bearing, c)
            if n + 1 < len(present):
                assert np.array_equal(grouped[first + count], point), (bearing, c)
            members = grouped[first:first + count]
            own = np.linalg.norm(members - point, axis=1).min()
            assert own > 1.0, "threshold not reached: category %d's own best is %.3g from the bait" % (c, own)
            if not bearing:
                continue
            # the bearing model matches by direction: the bearings in the sensor frame, as the kernels form them, against the detection's
            frame = ref.sensor_frame(tuple(state), ref.rotation_matrix(fam.TILTED[:4]).tolist(), list(fam.TILTED[4:]))
            d = ref._unit(tuple(fam._leak_vector(c, True)))
            cosine = lambda l: ref._dot3(ref._bearing_of(frame, tuple(float(v) for v in l)), d)
            assert cosine(point) > 1.0 - 1e-15  # the bait lies along the detection
            own = max(cosine(l) for l in members)
            assert own < fam.LEAK_COSINE, "threshold not reached: category %d's own best has the cosine %.3g with the bait" % (c, own)
    ks = {(c.bearing, c.k) for _, c in cases("range_leaks")}
    assert ks >= {(b, k) for b in (False, True) for k in fam.LEAK_KS}
    for _, case in cases("range_leaks"):
        if case.bearing and "absent" not in case.tag:
            assert list(case.dcat) == sorted(case.dcat, reverse=True)
    assert any(c.bearing and c.k == 64 and len(set(c.dcat.tolist())) == 1 for _, c in cases("range_leaks"))
    assert any(not c.bearing and set(fam.LEAK_ABSENT) <= set(c.dcat.tolist()) for _, c in cases("range_leaks"))


def test_tiny_weights_land_in_every_range():
    low, tiny, denormal_end = mpmath.mpf("1e-290"), mpmath.mpf(2) ** -1022, mpmath.mpf(2) ** -1075
    seen = dict(small=0, denormal=0, below=0, zero_terms=0)
    for number, case in cases("tiny_weights"):
        want = exact("tiny_weights", number)[0]
        got = case.loop()[0]
        seen["small"] += sum(low <= w <= mpmath.mpf("1e-200") for w in want)
        seen["denormal"] += sum(denormal_end < w < tiny for w in want)
        seen["below"] += sum(w < denormal_end for w in want)
        for g, w in zip(got, want):
            if w < denormal_end:
                assert g == 0.0 and not math.copysign(1.0, g) < 0, case.tag
        if "terms_underflow,rp=0" in case.tag:
            seen["zero_terms"] += int(np.sum(got == 0.0))
            assert want[-1] < mpmath.mpf("1e-1300")  # (each of the four terms is below the denormals)
        if "rp=1e-3" in case.tag:
            assert np.all(got >= case.w0 * 1e-3 ** case.k * (1 - 1e-12))  # (the floor holds)
    assert min(seen.values()) >= 2, "threshold not reached: %s" % seen


def test_degenerate_vectors_are_what_they_say():
    landmark, level, tilted = fam.degenerate_vectors()
    assert (landmark.det == 0).all(axis=1).sum() == 3 and (level.det == 0).all(axis=1).sum() == 1
    one = lambda case, state, d, c: float(ref.weights_exact(case.ref_map(), [state], [d], [c], [1.0], case.bearing, **case.params)[0][0])
    s = 1.25
    # the landmark model at the identity pose: category 1 is straight ahead (aperture 0), category 2 straight behind (aperture pi)
    assert one(landmark, landmark.states[0], (2.0, 0.0, 0.0), 1) == pytest.approx(math.exp(-4.0 / 4.5) + 1e-4, rel=1e-15)
    assert one(landmark, landmark.states[0], (2.0, 0.0, 0.0), 2) == pytest.approx(math.exp(-4.0 / 4.5) * math.exp(-math.pi**2 / (2 * s * s)) + 1e-4, rel=1e-15)
    # a landmark exactly at the robot, a zero detection: range error 0, aperture atan2(0, 0) = 0
    assert one(landmark, landmark.states[3], (0.0, 0.0, 0.0), 3) == 1.0 + 1e-4
    assert one(level, level.states[0], (1.0, 0.0, 0.0), 1) == 1.0
    assert one(level, level.states[0], (1.0, 0.0, 0.0), 2) == pytest.approx(math.exp(-math.pi**2 / (2 * s * s)), rel=1e-15)
    assert one(level, level.states[0], (0.0, 0.0, 1.0), 4) == 1.0  # the vertical bearing of the landmark overhead
    # the tilted sensor's origin: the landmark's bearing is the zero vector, whatever the detection
    for state, c in ((tilted.states[0], 3), (tilted.states[3], 6)):
        frame = ref.sensor_frame(tuple(state), ref.rotation_matrix(fam.TILTED[:4]).tolist(), list(fam.TILTED[4:]))
        assert [tuple(l) for l in tilted.positions[tilted.categories == c]] == [frame[1]]
        assert one(tilted, state, (0.5, -0.5, 0.25), c) == 1.0


# ---- the host plumbing, in a program of its own under the sanitizers ---------------------------------------------------------------------------
DRIVER = r"""
// driver <file>: kind, sigma_range, sigma_bearing, L, L lines "x y z category" (hex floats), k, k lines "x y z category".
// Prints the status of landmark_layout_map and its message; then the ranges, the grouped landmarks, the status of landmark_records
// and every record's first, count, place, range and unit vector.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "landmark_host.h"

using namespace mcl;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* in = std::fopen(argv[1], "r");
  if (!in) return 2;
  int kind;
  double sigma_range, sigma_bearing;
  unsigned long long L, k;
  if (std::fscanf(in, "%d %la %la %llu", &kind, &sigma_range, &sigma_bearing, &L) != 4) return 2;
  std::vector<double> positions(3 * L), xyz;
  std::vector<uint32_t> categories(L), dcat;
  for (unsigned long long i = 0; i < L; ++i)
    if (std::fscanf(in, "%la %la %la %" SCNu32, &positions[3 * i], &positions[3 * i + 1], &positions[3 * i + 2], &categories[i]) != 4) return 2;
  if (std::fscanf(in, "%llu", &k) != 1) return 2;
  xyz.resize(3 * k), dcat.resize(k);
  for (unsigned long long i = 0; i < k; ++i)
    if (std::fscanf(in, "%la %la %la %" SCNu32, &xyz[3 * i], &xyz[3 * i + 1], &xyz[3 * i + 2], &dcat[i]) != 4) return 2;
  std::fclose(in);
  mcl_landmark_params lp{sigma_range, sigma_bearing, 1e-4};
  mcl_bearing_params bp{sigma_bearing, {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0}};
  LandmarkMapLayout map;
  std::string error;
  const mcl_status ms = landmark_layout_map(kind, positions.data(), categories.data(), L, nullptr,
                                            kind == MCL_SENSOR_LANDMARK ? static_cast<const void*>(&lp) : static_cast<const void*>(&bp), &map, &error);
  std::printf("map %d %s\n", static_cast<int>(ms), error.c_str());
  if (ms != MCL_OK) return 0;
  std::printf("ranges %zu\n", map.ranges.size());
  for (const auto& r : map.ranges) std::printf("%" PRIu32 " %" PRIu32 " %" PRIu32 "\n", r.first, r.second.first, r.second.second);
  for (unsigned long long i = 0; i < L; ++i)
    std::printf("%a %a %a %a\n", map.landmarks[4 * i], map.landmarks[4 * i + 1], map.landmarks[4 * i + 2], map.landmarks[4 * i + 3]);
  std::vector<double> recs;
  error.clear();
  const mcl_status rs = landmark_records("driver", kind, xyz.data(), dcat.data(), k, &map.ranges, recs, &error);
  std::printf("records %d %s\n", static_cast<int>(rs), error.c_str());
  if (rs != MCL_OK) return 0;
  for (unsigned long long i = 0; i < k; ++i) {
    uint32_t packed[4];
    std::memcpy(packed, &recs[i * kLandmarkRecord + 7], sizeof packed);
    std::printf("%" PRIu32 " %" PRIu32 " %" PRIu32 " %a %a %a %a\n", packed[0], packed[1], packed[2], recs[i * kLandmarkRecord + 3],
                recs[i * kLandmarkRecord + 4], recs[i * kLandmarkRecord + 5], recs[i * kLandmarkRecord + 6]);
  }
  return 0;
}
"""
KIND = {False: 4, True: 5}  # MCL_SENSOR_LANDMARK, MCL_SENSOR_BEARING


@pytest.fixture(scope="module")
def plumbing(tmp_path_factory):
    from beluga_amd import capi
    assert (capi.MCL_SENSOR_LANDMARK, capi.MCL_SENSOR_BEARING) == (KIND[False], KIND[True])
    d = tmp_path_factory.mktemp("landmark_plumbing")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "landmark_plumbing_san"
    csrc = os.path.join(ROOT, "beluga_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc, "-I", os.path.join(ROOT, "include"), str(src),
                           os.path.join(csrc, "landmark_host.cpp"), "-o", str(exe)])

    def run(bearing, positions, categories, det, dcat, sigma_range=1.0, sigma_bearing=1.0):
        lines = ["%d %s %s %d" % (KIND[bearing], float(sigma_range).hex(), float(sigma_bearing).hex(), len(positions))]
        lines += ["%s %s %s %d" % (float(p[0]).hex(), float(p[1]).hex(), float(p[2]).hex(), int(c)) for p, c in zip(positions, categories)]
        lines += [str(len(det))] + ["%s %s %s %d" % (float(p[0]).hex(), float(p[1]).hex(), float(p[2]).hex(), int(c)) for p, c in zip(det, dcat)]
        path = d / "in.txt"
        path.write_text("\n".join(lines) + "\n")
        done = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        assert done.returncode == 0 and "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr, done.stderr
        return done.stdout.splitlines()

    return run


def test_host_plumbing_lays_out_the_range_leak_maps_as_restated(plumbing):
    """landmark_layout_map and landmark_records on every case of range_leaks (categories up to 0xFFFFFFFF, k up to 64, categories the map
    does not have): the ranges, the stable map order inside a category, each record's (first, count, place), range and unit vector are
    the restated ones, and `place` is a permutation."""
    checked = 0
    for _, case in cases("range_leaks"):
        out = plumbing(case.bearing, case.positions, case.categories, case.det, case.dcat)
        grouped, _, ranges = ref.layout(case.ref_map())
        assert out[0].split()[:2] == ["map", "0"] and out[1] == "ranges %d" % len(ranges)
        got_ranges = {int(c): (int(f), int(n)) for c, f, n in (row.split() for row in out[2:2 + len(ranges)])}
        assert got_ranges == ranges
        rows = out[2 + len(ranges):2 + len(ranges) + len(grouped)]
        got = np.array([[float.fromhex(v) for v in row.split()] for row in rows])
        assert np.array_equal(got[:, :3], grouped) and np.all(got[:, 3] == 0.0)
        for c, (first, count) in ranges.items():  # the map's order kept inside a category
            assert np.array_equal(grouped[first:first + count], case.positions[case.categories == np.uint32(c)])
        tail = out[2 + len(ranges) + len(grouped):]
        assert tail[0].split()[:2] == ["records", "0"] and len(tail) == 1 + case.k
        want = ref.records(case.ref_map(), case.dcat, case.bearing)
        places = []
        for row, (first, count, place) in zip(tail[1:], want):
            f = row.split()
            assert (int(f[0]), int(f[1]), int(f[2])) == (first, count, place), case.tag
            d = tuple(float(v) for v in case.det[place])
            assert float.fromhex(f[3]) == math.sqrt(ref._sq3(*d)) and tuple(float.fromhex(v) for v in f[4:7]) == ref._unit(d)
            places.append(place)
            checked += 1
        assert sorted(places) == list(range(case.k))
    assert checked > 250


def test_host_plumbing_takes_64_detections_and_refuses_65_and_degenerate_sigmas(plumbing):
    pos, cat = np.array([(1.0, 2.0, 0.5), (0.0, 1.0, 0.0)]), [3, 3]
    for bearing in (False, True):
        out = plumbing(bearing, pos, cat, np.ones((64, 3)), [3] * 64)
        assert out[0].split()[:2] == ["map", "0"] and out[-65].split()[:2] == ["records", "0"]
        out = plumbing(bearing, pos, cat, np.ones((65, 3)), [3] * 65)
        assert out[-1] == "records -1 driver: more than MCL_LANDMARK_MAX_DETECTIONS detections"
        # (2 sigma) sigma that underflows to 0 or overflows: -0 / 0 and inf / inf are NaN weights for finite inputs
        for sigma in (1e-170, 1e160):
            out = plumbing(bearing, pos, cat, np.ones((1, 3)), [3], sigma_bearing=sigma)
            assert out == ["map -1 mcl_set_landmark_map: (2 sigma) sigma must be positive and finite for " + ("sigma_bearing" if bearing else "sigma_range and sigma_bearing")]
        assert plumbing(bearing, pos, cat, np.ones((1, 3)), [3], sigma_bearing=1e-150)[0].split()[:2] == ["map", "0"]
    assert plumbing(False, pos, cat, np.ones((1, 3)), [3], sigma_range=1e-170)[0].startswith("map -1 mcl_set_landmark_map: (2 sigma) sigma")
