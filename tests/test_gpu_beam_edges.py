"""What the beam model's RAY WALKS are held to: every family of tests/beam_families.py through every kernel form it can reach, against the
cell-by-cell rule of tests/beam_reference.py, under parameters where one wrong hit cell moves a weight by more than 1e-6.

Forms: the wave-per-particle kernel (k_reweight_beam: n = 1, 3, 4, 5, 65 - four particles per workgroup; at n = 65 once per 65 states of
the case, so that every state of a case goes through it), the ordered kernel
(k_reweight_beam_sorted, beam_sort_min_particles = 0: it engages at any n; run at n = 1025 and 1024 + 27, i.e. a second workgroup of one
and of 27 live lanes) with beam_table 1 and 0 and all four combinations of beam_sectors x beam_free_ahead, and a fused batch member
(k_batch_reweight_beam) against its lone twin.  Each run is pinned by the counters beam_wave_launches / beam_ordered_launches: exactly the
expected one moves, by one.  The plain cast_ray arm of k_reweight_beam (`bits.fine == nullptr`) cannot be reached through the C ABI:
mcl_set_map always packs the non-free bits of a beam context's map.

Held: the cells visited EQUAL to the reference's count, per case and run; weights within 1e-10 of beam_reference (the project's beam bar:
libm differences in erf and exp, not the walk) with prior weights that are not 1; the four sectors x free-ahead combinations within 1e-12
of each other (the claim of test_beam_kernel_options_visit_the_same_cells_and_leave_the_same_weights); a batch member bit for bit its lone
twin; nothing written past n.

Why no address these kernels form can leave its buffer, for any pose and far end whose cells are below 2^31 and any line of fewer than 2^27
cells - mcl_reweight refuses a beam_max_range / resolution of 2^27 - 2 cells or more (kBeamMaxReachCells; asserted below) - (read off
csrc/beam_kernels.hip before the first run; it covers the sources and far ends outside the grid, the thin long grids and the poses outside
the window of the families):
  * A walk only ever covers cells 0 .. upto of its line, and upto comes from walk_room: -1 (no walk at all) when the source cell is outside
    the box, else the largest k whose cell is inside it on both axes - the major axis by subtraction, the minor axis by the first k at which
    the trip count leaves, in 64-bit arithmetic (floor_div's three ranges; its float range is corrected by the remainder, so it is exact).
    The box is the grid (cast_ray_grid, the whole-grid part of cast_ray_window) or the grid cut with the LDS window.  A source or far end
    outside the grid therefore gives an empty or a shortened walk, never a cell outside.
  * The unclamped examine_cells<false, false> and examine_column run only under `k + 8 <= upto`: cells k .. k + 7 are cells of the walk and
    cell k + 8 exists, all inside the box, so cy * fine_stride + (cx >> 5) is a word of the bit map (ceil(W / 32) words per row; kWinStride
    in LDS), and the two coarse words row[b0 >> 5], row[b1 >> 5] are those of the blocks of cell k and of cell k + 8 (minor_next is cell
    k + 8's minor coordinate: trips8 and rest8 are exact - 8 * dminor <= 16 * span stays an int below 2^31 under the library's bound, and
    the float quotient, at most 8, is corrected by its remainder).  The clamped examine_cells of phases 1 and 3 clamps the cells behind `count` into the map.
  * dist look-ups (clear_ahead, phase 2's d): always at the block of cell k <= upto, inside the box: the grid's map has ceil(H / 8) rows of
    dist_stride >= ceil(W / 8) bytes, the window's copy 128 x 128 with window coordinates in [0, 1023].  walk_advance_free and the
    block-distance skip read nothing; they move the position by cells that the `room` / `upto - k + 1` bounds keep at or before upto + 1.
  * Window staging: global reads are guarded (0 <= gy < H, 0 <= word < words_per_row; blocks of the distance map by `inside`), LDS writes go
    to row * kWinStride + col with row < 1024, col < 32 and to fixed ranges behind them.  The certificate reads dist only after checking
    0 <= px, py < 1024, and writes s_free_ahead[b - b_begin] only when a segment has at most kBeamCertified = 2048 beams (per_beam_entries;
    both `certified` and `sectors > 1` imply it) - the family with segments of 2049 beams takes neither.
  * table.entries[at]: at = min(r2, no_hit) and no_hit is the table's last index; r2 = cx^2 + cy^2 of a hit at most max_range + 1 cells
    away where a table exists (up to 2049 cells), and below 2^31 everywhere here (40 000-cell grids).
  * Scan points by b < B (the wave kernel's staged copy: B <= 4096, checked by mcl_reweight), poses through perm[t < n] (lanes past n
    repeat particle n - 1 and store nothing), partial[segment * n + t] with t < n.
"""
import numpy as np
import pytest

import beam_families as fam
import beam_reference as ref
from beluga_amd import capi
from beluga_amd.amcl import Amcl, AmclBatch, AmclParams, BeamModelParam, DifferentialDriveModelParam, OccupancyGrid, se2_from_xytheta

pytestmark = pytest.mark.gpu

MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
COUNTERS = ("beam_wave_launches", "beam_ordered_launches")
WAVE_SIZES = (1, 3, 4, 5, 65)
ORDERED_SIZES = (1025, 1024 + 27)
CAPACITY = max(ORDERED_SIZES) + 64
WAVE_MAX_POINTS = 4096
# form -> (set sizes, options, the counter that moves)
FORMS = {"wave": (WAVE_SIZES, {"beam_sort_min_particles": 1 << 30}, "beam_wave_launches")}
for table, sectors, ahead in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 0, 0)):
    FORMS["ordered_table%d_sectors%d_ahead%d" % (table, sectors, ahead)] = (
        ORDERED_SIZES if (table, sectors, ahead) == (1, 1, 1) else ORDERED_SIZES[:1],
        {"beam_sort_min_particles": 0, "beam_table": table, "beam_sectors": sectors, "beam_free_ahead": ahead}, "beam_ordered_launches")
SAME_WEIGHTS = [f for f in FORMS if f.startswith("ordered_table1")]  # sectors x free ahead: 1e-12


def grid_of(case):
    return OccupancyGrid(cells=case["cells"], resolution=case["resolution"], origin=case["origin"])


def run_form(f, case, r, form, n, offset=0):
    """Weights of n particles (fam.assignment's states, prior weights not 1) under `form`; holds the count, the pin and the rows past n."""
    _, options, moved = FORMS[form]
    idx = fam.assignment(case, CAPACITY, offset)
    w0 = np.random.Generator(np.random.MT19937(3)).uniform(0.5, 1.5, CAPACITY)
    for name, value in options.items():
        f.set_option(name, value)
    f.set_particles(case["states"][idx], w0)
    f.set_num_particles(n)
    before = {c: f.counter(c) for c in COUNTERS}
    f.beam_cells_visited(reset=True)
    f.reweight(case["points"])
    visited = f.beam_cells_visited()
    delta = {c: f.counter(c) - before[c] for c in COUNTERS}
    assert delta == {c: (1 if c == moved else 0) for c in COUNTERS}, (form, n, delta)
    if "majority" in case and moved == "beam_ordered_launches":
        # The case's claims are about windows around a majority pose: workgroup 0's middle particle is one, and so is the middle particle of
        # the workgroup that holds the pose at the sector window's edge and of one that holds a pose outside the window (a pose that sorts
        # last can be alone in the last workgroup - 1025 = 1024 + 1 -; that is at most one of the two outside poses).
        perm, _ = f.debug_order()
        place = np.empty(n, dtype=np.int64)
        place[perm] = np.arange(n)
        idx = np.asarray(idx)
        beside_majority = {int(idx[j]) for j in range(n) if idx[perm[min((place[j] // 1024) * 1024 + 512, n - 1)]] < case["majority"]}
        assert set(range(case["majority"])) <= beside_majority, (form, n, beside_majority)
        if n == ORDERED_SIZES[0]:  # (all five ordered forms; the run at 1024 + 27 is about the tail lanes: its last 27 of the order have the last as middle)
            assert beside_majority & set(case["outside"]), (form, n, beside_majority)
            assert case["edge_pose"] is None or case["edge_pose"] in beside_majority, (form, n, beside_majority)
    f.set_num_particles(CAPACITY)
    got = f.particles()[1]
    assert np.array_equal(got[n:], w0[n:]), "weights past n were written"
    want_cells = int(r["visited"].sum(axis=1)[idx[:n]].sum())
    want = r["weights"][idx[:n]] * w0[:n]
    err = float(np.max(np.abs(got[:n] - want) / want))
    print("beam_edges %s %s n=%d+%d B=%d cells=%d (want %d) worst=%.3g" % (case["targets"], form, n, offset, len(case["points"]), visited, want_cells, err))
    assert visited == want_cells, (case["targets"], form, n, visited, want_cells)
    assert err <= 1e-10, (case["targets"], form, n, err)
    return got[:n]


_filters, _references = {}, {}


def filter_for(case):
    """One filter per (grid, beam parameters), kept for the module (the parameters are fixed at mcl_create)."""
    key = (id(case["cells"]), tuple(case["origin"]), case["resolution"], tuple(case["params"]))
    if key not in _filters:
        _filters[key] = Amcl(grid_of(case), MOTION, BeamModelParam(*case["params"]), AmclParams(min_particles=CAPACITY, max_particles=CAPACITY), seed=11)
    return _filters[key]


def reference_for(case):
    key = (id(case["cells"]), id(case["states"]), tuple(case["params"]), case["points"].tobytes())
    if key not in _references:
        _references[key] = ref.reference(case)
    return _references[key]


@pytest.fixture(scope="module", autouse=True)
def _close_filters():
    yield
    for f in _filters.values():
        f.close()
    _filters.clear()
    _references.clear()


def check_case(case):
    r, f = reference_for(case), filter_for(case)
    results = {}
    for form, (sizes, _, _) in FORMS.items():
        if form == "wave" and len(case["points"]) > WAVE_MAX_POINTS:  # the wave kernel stages at most 4096 points: the scan is refused
            f.set_option("beam_sort_min_particles", 1 << 30)
            with pytest.raises(capi.MclError):
                f.reweight(case["points"])
            continue
        for n in sizes:
            results[(form, n)] = run_form(f, case, r, form, n)
        if form == "wave" and "majority" not in case:  # the states beyond the first 65, 65 at a time
            for offset in range(sizes[-1], len(case["states"]), sizes[-1]):
                run_form(f, case, r, form, sizes[-1], offset)
    base = results[(SAME_WEIGHTS[0], ORDERED_SIZES[0])]
    for form in SAME_WEIGHTS[1:]:
        np.testing.assert_allclose(results[(form, ORDERED_SIZES[0])], base, rtol=1e-12, atol=1e-300, err_msg=form)


def test_a_reach_of_2_to_the_27_cells_is_refused():
    """The walks keep 16 x the line's span in an int: mcl_reweight refuses beam_max_range / resolution from 2^27 - 2 cells on, the set
    untouched, and takes the largest reach below it."""
    case = fam.slopes()[0]
    for cells, refused in ((2.0 ** 27 - 2.0, True), (2.0 ** 27 - 3.0, False)):
        params = ref.revealing_params(fam.POW, cells * fam.POW)
        f = Amcl(OccupancyGrid(cells=case["cells"], resolution=fam.POW, origin=case["origin"]), MOTION, BeamModelParam(*params),
                 AmclParams(min_particles=5, max_particles=5), seed=11)
        states, w0 = case["states"][:5] * np.array([1.0, 1.0, fam.POW / fam.RES, fam.POW / fam.RES]), np.linspace(0.5, 1.5, 5)
        f.set_particles(states, w0)
        if refused:
            with pytest.raises(capi.MclError):
                f.reweight(case["points"])
            assert np.array_equal(f.particles()[1], w0) and f.counter("beam_wave_launches") == 0
        else:
            c = dict(case, resolution=fam.POW, states=states, params=params)
            r = ref.reference(c)
            f.reweight(case["points"])
            assert f.beam_cells_visited() == r["steps"]
            np.testing.assert_allclose(f.particles()[1], r["weights"] * w0, rtol=1e-10)
        f.close()


@pytest.mark.parametrize("name", sorted(n for n in fam.FAMILIES if n != "beam_counts"))
def test_every_form_walks_the_reference_cells(name):
    for case in fam.FAMILIES[name]():
        check_case(case)


def test_every_beam_count_and_segments_beyond_the_certificate():
    """B = 1, 7, 8, 9 (no segments below 16 beams), 63, 64, 65, 129 (partial sums and k_lf_combine), and 32 784 beams: 16 segments of 2049,
    more than kBeamCertified - reachable at these set sizes only with that many beams."""
    scan, many = fam.beam_counts()
    for B in fam.BEAM_COUNTS:
        check_case(fam.prefix(scan, B))
    check_case(many)


def test_a_fused_batch_member_is_its_lone_twin_and_both_are_the_reference():
    """mcl_batch_update with batch_beam_fused = 1 (k_batch_reweight_beam) against lone twins driven by mcl_update, bit for bit: states,
    weights, cells visited.  No resampling in the cycle, so the weights are the reweight's, normalised: against beam_reference on the
    propagated states, each within 1e-10 - the ratios to the reference agree within 2e-10 - and the count exactly."""
    cases = [fam.slopes()[7], fam.obstacle_at_k()[2], fam.borders_and_tiny_grids()[-2]]
    params = AmclParams(min_particles=65, max_particles=65, resample_interval=1000)
    specs = [dict(grid=grid_of(c), motion=MOTION, sensor=BeamModelParam(*c["params"]), params=params, seed=5 + k, options={"batch_beam_fused": 1})
             for k, c in enumerate(cases)]
    batch = AmclBatch(specs)
    twins = [Amcl(s["grid"], MOTION, s["sensor"], params, seed=s["seed"]) for s in specs]
    w0 = np.random.Generator(np.random.MT19937(4)).uniform(0.5, 1.5, 65)
    for k, c in enumerate(cases):
        states = c["states"][fam.assignment(c, 65)]
        for f in (batch.members[k], twins[k]):
            f.set_particles(states, w0)
            f.beam_cells_visited(reset=True)
    control = se2_from_xytheta(0.0, 0.0, 0.0)
    got = batch.update([control] * len(cases), [c["points"] for c in cases])
    assert batch.counter("members_beam_fused") == len(cases) and batch.counter("beam_launches") == 1
    for k, c in enumerate(cases):
        before = {name: twins[k].counter(name) for name in COUNTERS}
        want = twins[k].update(control, c["points"])
        assert {name: twins[k].counter(name) - before[name] for name in COUNTERS} == {"beam_wave_launches": 1, "beam_ordered_launches": 0}
        assert [batch.members[k].counter(name) for name in COUNTERS] == [0, 0]  # (the shared launch is the batch's beam_launches)
        assert want is not None and np.array_equal(got[k][0], want[0]) and np.array_equal(got[k][1], want[1], equal_nan=True)
        ms, mw = batch.members[k].particles()
        ts, tw = twins[k].particles()
        assert np.array_equal(ms, ts) and np.array_equal(mw, tw)
        cells = twins[k].beam_cells_visited(reset=False)
        assert batch.members[k].beam_cells_visited(reset=False) == cells
        r = ref.reference(c, states=ts)
        assert cells == r["steps"], (k, cells, r["steps"])
        ratio = tw / (r["weights"] * w0)
        assert ratio.max() / ratio.min() - 1.0 <= 2e-10, (k, ratio.max() / ratio.min() - 1.0)
    batch.close()
    for f in twins:
        f.close()
