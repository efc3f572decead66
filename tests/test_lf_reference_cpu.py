"""tests/lf_reference.py against the CPU oracle, and tests/lf_families.py against what each family claims.  No device.

KILLS: which restated wrong cell rule (lf_reference.MUTANTS) each family must expose - on at least 32 end-points, and in a weight on
the revealing field.  EQUIVALENT: mutants that pick the reference's cells on EVERY end-point a kernel can be handed, and why:
  * fma_no_guard - the fast kernels send a wave holding a particle 2^14 cells or more from the grid origin through the exact
    evaluation.  The host routes a launch to a fast kernel only for scans within 8192 cells of the sensor and grids below 2^14 cells per
    side (launch_reweight_lf), so that an end-point that can fall INSIDE the grid has |px ict|, |py ist| < 2^13 and |ixt| < 2^14 + 2^13
    whatever the guard: every term stays under 2^15 cells, the bound of 2^-35 cells on |v~ - v| holds, and the fallback's trigger of
    2^-33 covers it (long_lever puts particles at 16 383.5 and 16 384.5 cells and asserts that the two rules agree).  Farther particles'
    end-points are outside the grid by either rule.  The guard is redundant under the host's routing; it is kept, and tested to change
    nothing.
No family may kill nothing, and every other mutant is killed by at least one.
"""
import numpy as np
import pytest

import lf_families as fam
import lf_reference as ref
from oracle import binding as orc

MAX_LASER = 100.0
KILLS = {
    "ulp_straddle": ("nearest", "fma_no_fallback"),
    "trigger_ring": ("nearest", "fma_no_fallback", "fma_trigger_halved"),
    "long_lever": ("nearest", "fma_no_fallback", "fma_trigger_halved"),
    "borders": ("truncate", "nearest", "bounds_le", "fma_no_fallback"),
    "small_grids": ("truncate", "nearest", "bounds_le"),
    "beam_counts": ("nearest",),
    "no_cell": ("non_finite_is_cell_0", "wrap_mod_2_32"),
}
EQUIVALENT = ("fma_no_guard",)


def _cases(name):
    return fam.no_cell(True) if name == "no_cell" else fam.FAMILIES[name]()


def _args(c):
    return c["resolution"], c["origin"], c["states"], c["points"]


def _differs(rule, c, xi, yi, inside):
    mx, my, mi = rule(c["shape"], *_args(c))
    return (mi != inside) | (inside & ((mx != xi) | (my != yi)))


@pytest.mark.parametrize("name", sorted(fam.FAMILIES))
def test_reference_equals_the_oracle_and_every_family_kills_its_mutants(name):
    """Cells bit for bit, weights within (B + 1) 2^-53 relative (the oracle's own sum of B + 1 positive terms against the exact one).

    no_cell: static_cast<int> of NaN, +-inf or a floor beyond int is undefined in C++.  On this compiler (x86-64: cvttsd2si returns
    INT_MIN for all of them) the oracle's cast gives a negative cell, "not contained", which is what the written rule says - asserted
    here as a RECORD of the compiler's choice; the written rule of lf_reference.py is the contract, and it has no excluded cases."""
    killed = {m: 0 for m in ref.MUTANTS}
    weight_moved = {m: False for m in ref.MUTANTS}
    for c in _cases(name):
        H, W = c["shape"]
        B = len(c["points"])
        xi, yi, inside = ref.cells(c["shape"], *_args(c))
        ox, oy, oi = orc.lf_cells(c["shape"], *_args(c))
        assert np.array_equal(oi, inside)
        has = ref.cell_of(ref.end_points(*_args(c))[0])[1] & ref.cell_of(ref.end_points(*_args(c))[1])[1]
        assert np.array_equal(ox[has], xi[has]) and np.array_equal(oy[has], yi[has])
        if name == "no_cell":
            assert not inside[~has].any() and (~has).sum() >= len(c["pairs"])
            assert np.all((ox[~has] == np.iinfo(np.int32).min) | (oy[~has] == np.iinfo(np.int32).min))  # the compiler's choice
        else:
            assert has.all()
        for kind in ("palette", "cube"):
            field = ref.revealing_field(H, W, kind)
            want = ref.weights(field, *_args(c)[:2], MAX_LASER, *_args(c)[2:])
            got = orc.lf_weights(field, c["resolution"], c["origin"], MAX_LASER, c["states"], c["points"])
            assert np.max(np.abs(got - want) / want) <= (B + 1) * 2.0 ** -53
            wantp = ref.weights_prob(field, *_args(c)[:2], MAX_LASER, *_args(c)[2:])
            gotp = orc.lf_prob_weights(field, c["resolution"], c["origin"], MAX_LASER, c["states"], c["points"])
            np.testing.assert_allclose(gotp, wantp, rtol=1e-11)
        # the fast kernels' rule as they implement it (v~, the zero-low-word fallback, the guard) picks the reference's cells
        assert not _differs(ref.FAST_RULE, c, xi, yi, inside).any()
        field = ref.revealing_field(H, W, "palette")
        want = ref.weights(field, *_args(c)[:2], MAX_LASER, *_args(c)[2:])
        for m, rule in ref.MUTANTS.items():
            d = _differs(rule, c, xi, yi, inside)
            killed[m] += int(d.sum())
            if d.any():
                moved = ref.weights(field, *_args(c)[:2], MAX_LASER, *_args(c)[2:], rule=rule)
                # (a mutant that still finds a cell of the same value - `bounds_le` reading the clipped edge cell - moves no weight there)
                weight_moved[m] |= bool(np.any(np.abs(moved - want) / want > 1e-9))
    for m in KILLS[name]:
        assert killed[m] >= 32 and weight_moved[m], (name, m, killed[m])
    for m in EQUIVALENT:
        assert killed[m] == 0, (name, m, killed[m])
    assert len(KILLS[name]) > 0


def test_every_mutant_is_killed_or_listed_as_equivalent():
    assert set(m for ms in KILLS.values() for m in ms) | set(EQUIVALENT) == set(ref.MUTANTS)


def _margins(c):
    return ref.margins(*_args(c), pairs=[(i, b) for i, b, _, _ in c["pairs"]])


def test_ulp_straddle_sits_within_four_ulps_and_a_quarter_fools_the_fma_evaluation():
    total = fooled = 0
    offsets = set()
    for c in fam.ulp_straddle():
        m = _margins(c)
        for i, b, axis, j in c["pairs"]:
            for a in axis:
                assert m["ulps_" + a][i, b] == abs(j)
                assert (np.floor(m["v" + a][i, b]) == np.rint(m["v" + a][i, b])) == (j >= 0)  # at or above the boundary: its cell
            offsets.add((axis, j))
            total += 1
            fooled += any(np.floor(m["v" + a][i, b]) != np.floor(m["v" + a + "_fast"][i, b]) for a in axis)
    assert offsets == {(axis, j) for axis in ("x", "y", "xy") for j in range(-4, 5)}
    assert total >= 200 and 4 * fooled >= total, (fooled, total)


@pytest.mark.parametrize("name", ["trigger_ring", "long_lever"])
def test_ring_families_sit_either_side_of_the_trigger(name):
    """v~ (exact rational evaluation, one rounding per fma) at (1 -+ 2^-6) 2^-33 and (1 -+ 2^-6) 2^-32 from an integer, on both sides:
    the low word of v~ + 1.5 * 2^20 is zero exactly for those inside 2^-33.
    long_lever: the particles are 16 383.5 / 16 384.5 cells out and every term of the evaluation stays under 2^15 cells; the measured
    |v~ - v| stays under the derivation's 2^-35 cells."""
    seen = set()
    worst = 0.0
    for c in fam.FAMILIES[name]():
        m = _margins(c)
        T = ref.transforms(c["origin"], c["states"]) / c["resolution"]
        for i, b, axis, d in c["pairs"]:
            vt = m["v" + axis + "_fast"][i, b]
            off = vt - np.rint(vt)
            tol = 2.0 ** -41 if name == "trigger_ring" else 0.0
            assert abs(off - d) <= tol, (i, b, off, d)
            _, lo = ref.fast_cell(vt)
            assert (lo == 0) == (abs(d) < ref.TRIGGER)
            seen.add(d)
            worst = max(worst, abs(vt - m["v" + axis][i, b]))
            if name == "long_lever":
                px, py = c["points"][b]
                terms = np.abs([px * T[i, 0], py * T[i, 1], px * T[i, 1], py * T[i, 0], T[i, 2], T[i, 3]])
                assert terms.max() < 2.0 ** 15 and terms.max() > 2.0 ** 13.9
        if name == "long_lever":
            far = np.maximum(np.abs(T[:, 2]), np.abs(T[:, 3]))
            assert set(np.round(far[far > 1e4], 1)) == {16383.5, 16384.5}
            pts = np.abs(c["points"]).sum(axis=1).max() / c["resolution"]
            assert pts < 8192.0  # the host keeps such a scan on the fast kernels
    assert seen == set(fam.RING)
    assert worst < 2.0 ** -35, worst


def test_borders_reach_every_edge_from_both_sides():
    seen = set()
    for c in fam.borders()[:2]:
        H, W = c["shape"]
        vx, vy = ref.end_points(*_args(c))
        for i, b, axis, (k, j) in c["pairs"]:
            v = (vx if axis == "x" else vy)[i, b]
            side = W if axis == "x" else H
            name = {-1: "-1", 0: "0", side - 1: "side-1", side: "side"}[k]
            if j == "in":
                assert -1 < v < 0
            elif k <= 0:
                assert v == k if j == 0 else (k - 2.0 ** -40 < v < k) if j < 0 else (k < v < k + 2.0 ** -40)
            else:
                assert v == fam.stepped(k, j)
            seen.add((axis, name, j if j == "in" else int(np.sign(j))))
    for axis in "xy":
        for name in ("-1", "0", "side-1", "side"):
            assert {(axis, name, s) for s in (-1, 1)} <= seen
        assert {(axis, name, 0) for name in ("side-1", "side")} <= seen and (axis, "-1", "in") in seen
    # (v == -1 or == 0 EXACTLY is rare among the values a cancelling sum produces under rotation: the lattice case below has both)
    zero = fam.borders()[2]
    vx, vy = ref.end_points(*_args(zero))
    assert np.any(np.signbit(zero["points"]) & (zero["points"] == 0)) and np.any(vx == 0)  # products that are -0; sums that are 0
    xi, yi, inside = ref.cells(zero["shape"], *_args(zero))
    assert np.all(xi[vx == 0] == 0) and np.all(inside[(vx == 0) & (vy == 0)])
    assert np.any(vx == -1) and np.all(xi[vx == -1] == -1) and not inside[vx == -1].any()


def test_small_grids_and_counts_and_no_cell_are_what_they_claim():
    assert [c["shape"][::-1] for c in fam.small_grids()] == [(1, 1), (1, 9), (9, 1), (7, 9), (65, 63)]
    for c in fam.small_grids():
        xi, yi, inside = ref.cells(c["shape"], *_args(c))
        assert inside.any() and (~inside).any()
    assert set(fam.GROUP_OF_8_COUNTS) == set(range(42)) and len(fam.beam_counts()[0]["points"]) >= max(fam.SEGMENT_COUNTS + fam.LANE_COUNTS)
    for B, (segments, per, last) in {129: (2, 65, 64), 193: (3, 65, 63), 1009: (15, 68, 57), 1025: (16, 65, 50), 1041: (16, 66, 51)}.items():
        waves = (16411 + 63) // 64
        s = max(1, min(min((4096 + waves - 1) // waves, 16), B // 64))  # launch_reweight_lf (kLfMaxSegments = 16)
        assert (s, -(-B // s), B - (s - 1) * -(-B // s)) == (segments, per, last)
    for gpu in (False, True):
        for c in fam.no_cell(not gpu):
            vx, vy = ref.end_points(*_args(c))
            has = ref.cell_of(vx)[1] & ref.cell_of(vy)[1]
            bad = sorted({b for _, b, _, _ in c["pairs"]})
            assert bad and not has[:, bad].any() and has[:, [b for b in range(len(c["points"])) if b not in bad]].all()
            if gpu:  # what the device is handed: only points the host can settle for every pose
                assert not np.isfinite(c["points"][bad]).all(axis=1).any()
    places = [sorted({b for _, b, _, _ in c["pairs"]}) for c in fam.no_cell()]
    assert [0] in places and [40] in places and [3] in places  # first, last, inside a group of 8


HOST_CHECK = r"""
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <random>
#include "cycle_host.h"
int main() {
  std::mt19937_64 g(1);
  std::uniform_real_distribution<double> ang(-3.2, 3.2), sc(0.999999, 1.000001), any(-10, 10);
  long bad = 0;
  for (long i = 0; i < 4000000; ++i) {
    double x, y;
    if (i & 1) { const double a = ang(g), s = sc(g); x = std::cos(a) * s; y = std::sin(a) * s; }
    else { x = any(g); y = any(g); }
    if (mcl::hypot_ieee(x, y) != std::hypot(x, y)) ++bad;
  }
  for (const double x : {0.0, -0.0, 1.0, HUGE_VAL, 1e-320, 1e300})
    for (const double y : {0.0, 3.0, -HUGE_VAL, 1e-310, 1e305})
      if (mcl::hypot_ieee(x, y) != std::hypot(x, y)) ++bad;
  if (!std::isnan(mcl::hypot_ieee(NAN, 1.0))) ++bad;
  const float u = static_cast<float>(1.0 / 100.0);
  const double pz = u;
  if (mcl::lf_acc0(false, u, 0) != 1.0 || mcl::lf_acc0(true, u, 0) != 0.0) ++bad;
  if (mcl::lf_acc0(false, u, 7) != 1.0 + 7.0 * (pz * pz * pz) || mcl::lf_acc0(true, u, 7) != 7.0 * std::log(pz)) ++bad;
  std::printf("%ld\n", bad);
  return bad != 0;
}
"""


def test_device_hypot_is_the_host_librarys_and_the_sums_start_where_the_rule_says(tmp_path):
    """csrc/se2.h hypot_ieee (what the kernels normalise rotations with) against std::hypot on 4M arguments - rotations scaled by
    1 +- 1e-6 and general ones - and on zeros, infinities, subnormals, NaN; csrc/cycle_host.h lf_acc0 (FieldView::acc0): exactly the model's
    start for a scan without dropped points, the start plus count x the unknown-space term otherwise."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "host_check.cpp"
    src.write_text(HOST_CHECK)
    exe = tmp_path / "host_check"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(root, "beluga_amd", "csrc"),
                           "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.strip() == "0"
