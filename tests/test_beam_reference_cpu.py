"""tests/beam_reference.py against the CPU oracle, and tests/beam_families.py against what each family claims.  No device.

KILLS: which restated wrong rule (beam_reference.MUTANTS) each family must expose - in a hit cell or a count of visited cells, and in a
weight by more than 1e-6 relative under beam_reference.revealing_params.  No family may kill nothing, and every mutant is killed by at
least one family; EQUIVALENT (mutants no input in contract can tell from the rule) is empty.
"""
import math

import numpy as np
import pytest

import beam_families as fam
import beam_reference as ref
from oracle import binding as orc

KILLS = {
    "slopes": ("trip_ge", "past_the_end", "stop_early", "modified", "unknown_free"),
    "obstacle_at_k": ("trip_ge", "stop_early", "modified", "unknown_free"),
    "borders_and_tiny_grids": ("truncate", "outside_hit", "unknown_free", "modified"),
    "cell_boundaries": ("truncate", "divide"),
    "closed_form_thresholds": ("outside_hit",),
    "window_and_sectors": ("unknown_free", "trip_ge"),
    "free_ahead": ("unknown_free", "modified"),
    "range_terms": ("short_le", "corners", "tie_sqrt"),
    "beam_counts": ("trip_ge", "outside_hit"),
}
EQUIVALENT = ()

_reference = {}


def reference(name, k):
    if (name, k) not in _reference:
        _reference[(name, k)] = ref.reference(fam.FAMILIES[name]()[k])
    return _reference[(name, k)]


def oracle_args(c):
    return c["cells"], c["resolution"], c["origin"], c["params"], c["states"], c["points"]


@pytest.mark.parametrize("name", sorted(fam.FAMILIES))
def test_reference_equals_the_oracle_and_every_family_kills_its_mutants(name):
    """The count of visited cells exactly (per pose: one oracle call each), the weights within the suite's 1e-10 (the oracle's libm erf and
    exp against extended precision), hit and range bit for bit on a sample of rays through orc.ray_cast."""
    killed = {m: 0 for m in KILLS[name]}
    moved = {m: 0.0 for m in KILLS[name]}
    for k, c in enumerate(fam.FAMILIES[name]()):
        r = reference(name, k)
        got, steps = orc.beam_weights(*oracle_args(c), return_steps=True)
        assert steps == r["steps"], (name, k, steps, r["steps"])
        np.testing.assert_allclose(got, r["weights"], rtol=1e-10, atol=1e-300, err_msg="%s[%d]" % (name, k))
        m, B = r["visited"].shape
        for i in range(0, m, max(1, m // 6)):  # per-pose counts: a compensating pair of errors would pass the total
            _, s = orc.beam_weights(c["cells"], c["resolution"], c["origin"], c["params"], c["states"][i:i + 1], c["points"], return_steps=True)
            assert s == int(r["visited"][i].sum()), (name, k, i)
        for m_ in KILLS[name]:
            x = ref.reference(c, m_)
            differs = (x["has_hit"] != r["has_hit"]) | (r["has_hit"] & (x["hit"] != r["hit"]).any(axis=2)) | (x["visited"] != r["visited"]) | \
                (x["short"] != r["short"])
            killed[m_] += int(differs.sum())
            moved[m_] = max(moved[m_], float(np.max(np.abs(x["weights"] - r["weights"]) / r["weights"])))
    for m_ in KILLS[name]:
        assert killed[m_] >= 1 and moved[m_] > 1e-6, (name, m_, killed[m_], moved[m_])
    assert len(KILLS[name]) > 0


def test_every_mutant_is_killed_or_listed_as_equivalent():
    assert set(m for ms in KILLS.values() for m in ms) | set(EQUIVALENT) == set(ref.MUTANTS)
    assert set(KILLS) == set(fam.FAMILIES)


def test_the_trace_is_the_oracles_bit_for_bit():
    """Both Bresenham variants, every octant, degenerate lines, negative coordinates."""
    rng = np.random.Generator(np.random.MT19937(1))
    ends = [(0, 0, 0, 0), (3, 4, 3, 4), (0, 0, 7, 0), (0, 0, 0, -7), (0, 0, 5, 5), (0, 0, -5, 5), (2, 1, 9, 7), (-3, -8, 4, -2), (0, 0, 8, 7), (0, 0, 7, 8)]
    ends += [tuple(int(v) for v in rng.integers(-40, 40, 4)) for _ in range(300)]
    for x0, y0, x1, y1 in ends:
        for modified in (False, True):
            want = orc.bresenham((x0, y0), (x1, y1), modified=modified)
            got = np.array(list(ref.line(x0, y0, x1, y1, modified=modified)), dtype=np.int32).reshape(-1, 2)
            assert np.array_equal(got, want), (x0, y0, x1, y1, modified)


@pytest.mark.parametrize("name", sorted(fam.FAMILIES))
def test_hit_and_range_are_the_oracles_bit_for_bit(name):
    """orc.ray_cast takes the bearing as an angle, so the rays are rebuilt from angles - nine fixed ones and those of the case's own first
    beams, which aim at what the case engineers - and both sides form the bearing the same way (cos and sin of the angle: the reference's
    so2_exp).  Every case of every family, up to eight poses of each; every family has rays that hit."""
    hits = 0
    for k, c in enumerate(fam.FAMILIES[name]()):
        angles = [0.0, 0.3, math.pi / 4, math.pi / 2, 2.0, math.pi, -2.5, -math.pi / 2, -0.4]
        angles += [math.atan2(float(py), float(px)) for px, py in c["points"][:12]]
        max_range = c["params"][6]
        T = ref.source_poses(c["origin"], c["states"])
        mask = ref.nonfree_mask(c["cells"])
        H, W = c["cells"].shape
        for i in range(0, len(T), max(1, -(-len(T) // 8))):
            Ti = [float(v) for v in T[i]]
            sx, sy = ref.cell_near(Ti[2], c["resolution"]), ref.cell_near(Ti[3], c["resolution"])
            for a in angles:
                ex, ey = ref.far_end(Ti, math.cos(a), math.sin(a), max_range)
                hit, _ = ref.cast(mask, W, H, sx, sy, ref.cell_near(ex, c["resolution"]), ref.cell_near(ey, c["resolution"]))
                want = orc.ray_cast(c["cells"], c["resolution"], c["origin"], c["states"][i], max_range, a)
                got = None if hit is None else ref.cell_distance(sx, sy, hit[0], hit[1], c["resolution"], max_range)
                assert got == want, (name, k, i, a, got, want)
                hits += hit is not None
    assert hits >= 20, (name, hits)


def test_extended_erf_and_the_revealing_parameters():
    xs = np.array([-7.5, -6.6, -3.0, -0.5, 0.0, 1e-9, 0.3, 1.0, 2.5, 4.0, 5.9, 6.5, 6.99, 7.0, 9.0])
    got = ref.to_f64(ref.x_erf(ref.ext(xs)))
    want = np.array([math.erf(v) for v in xs])
    assert np.max(np.abs(got - want)) <= 2.0 ** -52
    p = ref.revealing_params(0.05, 10.0)
    assert p[4] == 0.05 and p[3] <= 0.001 and p[6] == 10.0


# ---- what the families claim -----------------------------------------------------------------------------------------------------------
def _spans(r):
    """(major span, minor span, steep, major step sign, minor step sign) per ray."""
    d = r["far"] - r["source"][:, None, :]
    ax, ay = np.abs(d[..., 0]), np.abs(d[..., 1])
    steep = ax < ay
    return np.where(steep, ay, ax), np.where(steep, ax, ay), steep, np.sign(np.where(steep, d[..., 1], d[..., 0])), np.sign(np.where(steep, d[..., 0], d[..., 1]))


def test_slopes_cover_octants_lengths_and_block_phases():
    octants, majors, phases = set(), set(), set()
    axis = diagonal = plus_one = same_cell = 0
    for k, c in enumerate(fam.slopes()):
        r = reference("slopes", k)
        major, minor, steep, smaj, smin = _spans(r)
        if c.get("past_end"):  # beam 0: the cell behind the far-end cell is not free and nearer than max_range - and is not looked at
            past = r["far"][:, 0] + (1, 0)
            assert all(c["cells"][y, x] != 0 for x, y in past) and not r["has_hit"][:, 0].any()
            assert all(ref.cell_distance(*r["source"][i], *past[i], c["resolution"], math.inf) < c["params"][6] for i in range(len(past)))
            continue
        for i in range(major.shape[0]):
            for b in range(major.shape[1]):
                if minor[i, b] > 0:
                    octants.add((bool(steep[i, b]), int(smaj[i, b]), int(smin[i, b])))
                phases.add((int(r["source"][i, 0]) & 7, int(r["source"][i, 1]) & 7, int(smaj[i, b]), bool(steep[i, b])))
        majors |= set(int(v) for v in np.unique(major))
        axis += int(((minor == 0) & (major > 0)).sum())
        diagonal += int(((minor == major) & (major > 0)).sum())
        plus_one += int((major == minor + 1).sum())
        same_cell += int((major == 0).sum())
    assert len(octants) == 8
    assert set(range(0, 18)) | {23, 24, 25, 63, 64, 65} <= majors, sorted(majors)
    assert axis >= 64 and diagonal >= 64 and plus_one >= 64 and same_cell >= 64
    assert {(x, y, s, st) for x in range(8) for y in range(8) for s in (-1, 1) for st in (False, True)} <= phases


def test_obstacle_at_k_hits_every_index_of_every_line():
    xs7, xs31 = set(), set()
    for k, c in enumerate(fam.obstacle_at_k()):
        r = reference("obstacle_at_k", k)
        per_row, tile = c["tile"]
        trace = c["trace"]
        assert len(trace) >= 22
        seen = set()
        for i, kind in enumerate(c["kinds"]):
            ox, oy = (i % per_row) * tile, (i // per_row) * tile
            if isinstance(kind, int):
                assert r["has_hit"][i, 0] and r["visited"][i, 0] == kind + 1
                assert tuple(r["hit"][i, 0]) == (ox + trace[kind][0], oy + trace[kind][1])
                if kind == 0:
                    assert r["expected"][i, 0] == 0.0
                seen.add(kind)
                xs7.add(int(r["hit"][i, 0, 0]) & 7)
                xs31.add(int(r["hit"][i, 0, 0]) & 31)
            else:  # one past the end, beside the trace, the corner pair: beam 0 passes
                assert not r["has_hit"][i, 0] or r["visited"][i, 0] > len(trace), (k, kind)
        assert seen == set(range(len(trace)))
        assert {"past", "beside"} <= set(c["kinds"])
    assert any("corner" in c["kinds"] for c in fam.obstacle_at_k())
    assert {0, 7} <= xs7 and {0, 31} <= xs31


def test_borders_reach_every_side_corner_and_outside_source():
    sizes = []
    for k, c in enumerate(fam.borders_and_tiny_grids()):
        W, H = c["size"]
        sizes.append((W, H))
        r = reference("borders_and_tiny_grids", k)
        sx, sy = r["source"][:, 0], r["source"][:, 1]
        outside = (sx < 0) | (sy < 0) | (sx >= W) | (sy >= H)
        assert r["visited"][outside].sum() == 0 and outside.sum() >= 6 and (~outside).sum() >= 4
        assert {-1} <= set(sx[outside]) | set(sy[outside]) and (W in set(sx)) and (H in set(sy))
        assert (sx < -40).any() and (sy > H + 40).any()
        assert ((r["far"][..., 0] < 0) | (r["far"][..., 0] >= W)).any()
        if (W, H) == (157, 203) and not (c["cells"] == ref.UNKNOWN).all(axis=1).any():
            # exits through each side: the last visited cell of a ray without a hit that was cut by the grid
            exits = set()
            for i in np.nonzero(~outside)[0]:
                for b in range(r["visited"].shape[1]):
                    cells_ = list(ref.line(*r["source"][i], *r["far"][i, b]))
                    n_in = int(r["visited"][i, b])
                    if not r["has_hit"][i, b] and n_in < len(cells_):
                        x, y = cells_[n_in]
                        exits.add(("left" if x < 0 else "right" if x >= W else "") + ("low" if y < 0 else "high" if y >= H else ""))
            assert {"left", "right", "low", "high"} <= exits and any(len(e) > 5 for e in exits), exits  # (a corner: both at once)
    assert set(sizes) == set(fam.TINY_GRIDS)
    assert any((c["cells"][0] == ref.UNKNOWN).all() for c in fam.borders_and_tiny_grids())


def test_cell_boundaries_sit_on_and_next_to_their_boundary():
    for k, c in enumerate(fam.cell_boundaries()):
        r = reference("cell_boundaries", k)
        T = ref.source_poses(c["origin"], c["states"])
        inv = 1.0 / c["resolution"]
        sides = set()
        for i, axis, bound, what, side in c["marks"]:
            if what == "source":
                v, cell = float(T[i, 2 + axis]) * inv, int(r["source"][i, axis])
            else:
                ex = ref.far_end([float(t) for t in T[i]], *((1.0, 0.0) if axis == 0 else (0.0, 1.0)), c["params"][6])
                v, cell = ex[axis] * inv, int(r["far"][i, axis, axis])
            assert abs(v - bound) <= 2.0 ** -36, (k, i, v, bound)
            assert (v < bound, v == bound, v > bound) == (side == "below", side == "at", side == "above")
            assert cell == (bound - 1 if side == "below" else bound)
            sides.add((axis, bound, what, side))
        for axis in (0, 1):
            for what, bounds in (("source", (8, 32)), ("far", (32, 33))):  # (a far end on boundary 8 would have its source outside)
                assert {(axis, b, what, s) for b in bounds for s in ("below", "above")} <= sides
            assert (axis, 0, "source", "below") in sides  # floor -1, truncation 0


def test_threshold_cases_reach_the_ranges_they_name():
    seen, trips = set(), set()
    cases = fam.closed_form_thresholds()
    for k, c in enumerate(cases[:-1]):
        r = reference("closed_form_thresholds", k)
        H, W = c["cells"].shape
        major, minor, steep, _, _ = _spans(r)
        assert (major[:, 0] == c["span"]).all() and (steep[:, 0] == c["steep"]).all() and (minor[:, 0] > 0).all()
        for i in range(len(c["states"])):
            num = fam.exit_numerator(*r["source"][i], *r["far"][i, 0], W, H)
            assert num == (2 * c["room"] + 1) * c["span"], (k, i, num)
            seen.add((c["steep"], num, fam.floor_div_range(num)))
        assert (2 * major[:, 0] < (1 << 16)).all() == (c["span"] < 32768)
        assert major.max() + 2 < (1 << 27)  # (the library's bound on beam_max_range / resolution)
        # walk_trips_at's numerator at the hits (walk_seek): the third beam's hit in the border strip carries the case's range
        for i, b in zip(*np.nonzero(r["has_hit"])):
            trips.add((c["what"], fam.floor_div_range(fam.trips_numerator(*r["source"][i], *r["far"][i, b], int(r["visited"][i, b]) - 1))))
        assert r["has_hit"][2:, 2].all()
    for steep in (False, True):
        assert {(steep, (1 << 22) - 1, 0), (steep, 1 << 22, 1), (steep, (1 << 22) + 1, 1), (steep, (1 << 32) - 4, 1), (steep, (1 << 32) + 29, 2)} <= seen
    assert {("closed forms on", 0), ("closed forms off", 0), ("2^22", 1), ("2^32 - 4", 1), ("2^32 - 4", 2), ("2^32 + 29", 2)} <= trips, sorted(trips)
    # the block distances: Chebyshev, in blocks, from the ray's blocks to the one block that holds something
    c, r = cases[-1], reference("closed_form_thresholds", len(cases) - 1)
    bx, by = c["block"]
    assert c["cells"][8 * by:8 * by + 8, 8 * bx:8 * bx + 8].any() and (c["cells"] != 0).sum() == 1
    lengths = set()
    for i, d in enumerate(c["distances"]):
        cells_ = list(ref.line(*r["source"][i], *r["far"][i, 0]))[:int(r["visited"][i, 0])]
        assert min(min(max(abs((x >> 3) - bx), abs((y >> 3) - by)), 17) for x, y in cells_) == d
        assert r["has_hit"][i, 0] == (d == 0)
        lengths.add((d, len(cells_) & 7))
    assert {d for d, _ in lengths} == {0, 1, 2, 3, 16, 17} and len({l for d, l in lengths if d == 2}) == 8  # every remainder of the walk


def test_window_cases_hit_either_side_of_the_window_and_name_their_sectors():
    assert [fam.sectors_of(reach * fam.RES, fam.RES) for reach in fam.WINDOW_REACHES] == [1, 4, 4, 4, 1]
    for k, c in enumerate(fam.window_and_sectors()):
        r = reference("window_and_sectors", k)
        H, W = c["cells"].shape
        assert W > fam.WIN and H > fam.WIN
        x0, y0 = c["window"]
        assert (r["source"][:c["majority"]] == c["middle"]).all() and fam.window_of(*c["middle"]) == (x0, y0)
        for i in c["outside"]:                                                   # poses outside the window altogether
            sx, sy = r["source"][i]
            assert not (x0 <= sx < x0 + fam.WIN and y0 <= sy < y0 + fam.WIN)
        assert (c["edge_pose"] is not None) == (fam.sectors_of(c["params"][6], c["resolution"]) == 4)
        if c["edge_pose"] is not None:  # inside the +x +y sector's window, its rays hit that window's first column and the one outside it
            e, sx0 = c["edge_pose"], fam.sector_window_x0(c["middle"][0], c["reach"])
            assert 0 < r["source"][e, 0] - sx0 < 32
            assert {sx0, sx0 - 1} <= set(r["hit"][e][r["has_hit"][e]][:, 0]), (k, sx0)
        hx, hy = r["hit"][:6][r["has_hit"][:6]].T
        if c["reach"] >= 600:
            assert {x0 - 1, x0, x0 + fam.WIN - 1, x0 + fam.WIN} <= set(hx) and {y0 - 1, y0, y0 + fam.WIN - 1, y0 + fam.WIN} <= set(hy)
        T = ref.source_poses(c["origin"], c["states"])
        assert (T[:6, 0] == 1.0).all() and (T[:6, 1] == 0.0).all()               # the middle ray of beams 0 .. 3 lies on a seam
        z, bc, bs = zip(*[ref.bearing_of(*p) for p in c["points"][:4]])
        assert bs[0] == 0.0 and bc[1] == 0.0 and bs[2] == 0.0 and bc[3] == 0.0
        idx = fam.assignment(c, 1025)
        assert (idx < 6).sum() == 1025 - 6 and set(range(6, 12)) <= set(idx)


def test_free_ahead_cases_have_pillars_on_some_lanes_only():
    tight, wide = fam.free_ahead()
    r = reference("free_ahead", 0)
    assert (np.ptp(r["source"], axis=0) == 0).all()
    split = [b for b in range(r["visited"].shape[1]) if len({tuple(h) for h in r["hit"][:, b]}) > 1]
    assert len(split) >= 3                                                       # a pillar on some poses' ray, off the others'
    walls = r["expected"][0] / fam.RES
    assert walls.min() < 25 and walls.max() > 100
    assert np.ptp(reference("free_ahead", 1)["source"], axis=0).min() > 64


def test_range_terms_tie_clamp_and_saturate():
    for k, c in enumerate(fam.range_terms()):
        r = reference("range_terms", k)
        sigma, max_range = c["params"][4], c["params"][6]
        assert len(c["ties"]) >= 60
        for i, b, j in c["ties"]:
            e, z = r["expected"][i, b], r["z"][b]
            assert r["has_hit"][i, b] and z == (np.nextafter(e, 0.0), e, np.nextafter(e, np.inf))[j + 1]
            assert r["short"][i, b] == (j < 0)
        assert [bool(r["z"][b] < max_range) for b in c["tails"]] == [True, False, False, False]
        assert (r["expected"][-1] == 0.0).all() and (r["visited"][-1] == 1).all()  # the pose inside a non-free cell
        e = r["expected"][r["has_hit"]]
        lo, hi = 6.5 * math.sqrt(2.0) * sigma, 6.6 * math.sqrt(2.0) * sigma
        assert (e < lo).any() and ((e > lo) & (e < hi)).any() and (e > hi).any()
        if k == 0:
            assert ((max_range - e < lo) & (e < max_range)).any() and ((max_range - e > lo) & (max_range - e < hi)).any()
            # hits whose cell centres are max_range or more apart: fmin decides
            far = [(i, b) for i, b in zip(*np.nonzero(r["has_hit"])) if
                   ref.cell_distance(*r["source"][i], *r["hit"][i, b], c["resolution"], math.inf) >= max_range]
            assert len(far) >= 3 and all(r["expected"][i, b] == max_range for i, b in far)
        assert (math.ceil(c["reach"]) + 3 > 2046) == (k == 1)                    # beam_table_entries: no table for the second case


def test_beam_counts_are_what_the_launcher_splits():
    scan_, many = fam.beam_counts()
    assert len(scan_["points"]) >= max(fam.BEAM_COUNTS) and len(many["points"]) == fam.CERTIFIED_OVERFLOW
    for B, per in ((1, 1), (7, 7), (8, 8), (9, 9), (63, 9), (64, 8), (65, 9), (129, 9), (fam.CERTIFIED_OVERFLOW, 2049)):
        groups = 2  # 1025 or 1051 particles
        segments = max(1, min(min((512 + groups - 1) // groups, 16), B // 8))  # launch_reweight_beam (kLfMaxSegments = 16)
        assert -(-B // segments) == per, (B, segments)
