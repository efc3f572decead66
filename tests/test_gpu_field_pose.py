"""Option lf_pose_ahead: the likelihood-field kernels load world_to_field * pose, stored per particle by the propagation that wrote the pose
(or by k_field_pose, for a set nothing has propagated), instead of forming the product per particle and launch.  The same expression on
the same values: the weights are held EQUAL (==) between the two arms, on a small map whose origin is rotated and offset, for every
kernel form the option tables route to - pinned by the launch counters, as tests/test_gpu_lf_edges.py pins them - and along the
sequences that set and void the fact "field poses current" (set_facts.h), each also against a fresh context given the same particles.
The counter field_pose_rebuilds says where k_field_pose ran: exactly once in front of a reweight whose set no propagation of the
current map has written, never in the steady propagate -> reweight cycle, never with the option off."""
import numpy as np
import pytest

import lf_reference as ref
from beluga_amd.amcl import (Amcl, AmclBatch, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam,
                             LikelihoodFieldProbModelParam, OccupancyGrid, SharedMap, se2_from_xytheta)

pytestmark = pytest.mark.gpu

MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
LF = LikelihoodFieldModelParam(2.0, 100.0, 0.5, 0.5, 0.2, True)
LF_PROB = LikelihoodFieldProbModelParam(2.0, 100.0, 0.5, 0.5, 0.2, True)
H, W, RES = 80, 96, 0.05
ORIGIN = se2_from_xytheta(1.3, -0.7, 0.4)     # world_to_field is not the identity
ORIGIN_2 = se2_from_xytheta(-0.45, 0.9, -1.1)  # ... and the map swapped in has another one
N_PATCH = 448 * 2 + 5  # two full blocks of the patch kernel and a ragged one
N_WAVE = 64 * 3 + 1    # the wave-per-particle forms: three full waves' worth of particles and one more
BEAMS = (8, 9, 264)    # one group of 8, a tail, and (ordered kernels, below 4096 waves) four segments of 66
COUNTERS = ("lf_beams_launches", "lf_fast_launches", "lf_patch_launches", "lf_queue_launches", "lf_far_launches", "lf_far_beams_launches")
DEFAULTS = {"lf_variant": 2, "lf_table": 0, "lf_fast": 1, "lf_patch": 1, "lf_far_tiles": 1, "lf_dispersed": 2, "key_layout": 0,
            "lf_far_beams_per_wave": 0, "lf_small_particles": 512, "sort_min_particles": 512, "lf_queue": 1, "lf_queue_grid": 0}
PATCH = ("lf_fast_launches", "lf_patch_launches")
# form -> (particles, options, counters that move by one, field kind); "queue": the queue form takes single-segment launches only
FORMS = {
    "beams": (N_WAVE, {}, ("lf_beams_launches",), "palette"),
    "beams_variant3": (N_WAVE, {"lf_variant": 3}, ("lf_beams_launches",), "palette"),
    "index_order": (N_WAVE, {"lf_table": 1}, (), "cube"),
    "index_order_variant1": (N_WAVE, {"lf_variant": 1}, (), "palette"),
    "sorted_cube": (N_PATCH, {"lf_table": 1}, (), "cube"),
    "palette_exact": (N_PATCH, {"lf_fast": 0, "lf_patch": 0}, (), "palette"),
    "palette_fast": (N_PATCH, {"lf_patch": 0, "lf_far_tiles": 0, "lf_dispersed": 0}, ("lf_fast_launches",), "palette"),
    "palette_far": (N_PATCH, {"lf_patch": 0, "lf_far_tiles": 2, "lf_dispersed": 0}, ("lf_fast_launches", "lf_far_launches"), "far"),
    "far_beams": (N_PATCH, {"lf_patch": 0, "lf_far_tiles": 2, "lf_dispersed": 2},
                  ("lf_fast_launches", "lf_far_launches", "lf_far_beams_launches"), "far"),
    "patch": (N_PATCH, {"lf_patch": 2, "lf_queue": 0}, PATCH, "palette"),
    "patch_queue": (N_PATCH, {"lf_patch": 2, "lf_queue": 1, "lf_queue_grid": 2}, PATCH + ("lf_queue_launches",), "palette"),
}
PROB_FORMS = ("beams", "palette_fast", "far_beams", "patch", "patch_queue")


def grid_at(origin):
    """Scattered obstacles: the field the library builds from them differs from cell to cell, so a pose in the wrong frame shows."""
    cells = np.zeros((H, W), dtype=np.int8)
    cells[np.random.Generator(np.random.MT19937(17)).random((H, W)) < 0.03] = 100
    return OccupancyGrid(cells=cells, resolution=RES, origin=origin)


def field(kind):
    if kind != "far":
        return ref.revealing_field(H, W, kind)
    f = ref.revealing_field(H, W, "palette").copy()
    f[:, W // 2:] = np.float32(0.71875)  # flat: the far-tile bitmap has tiles to mark
    return f


def compose(a, b):
    """a * b of (cos, sin, x, y) rows (b may be many)."""
    b = np.atleast_2d(b)
    return np.stack([a[0] * b[:, 0] - a[1] * b[:, 1], a[1] * b[:, 0] + a[0] * b[:, 1], a[2] + a[0] * b[:, 2] - a[1] * b[:, 3],
                     a[3] + a[1] * b[:, 2] + a[0] * b[:, 3]], axis=1)


def cloud(n, origin=ORIGIN, seed=5):
    """n poses in the world whose field-frame poses sit around the middle of the grid, close enough for LDS patches to fit, and prior
    weights that are not 1."""
    rng = np.random.Generator(np.random.MT19937(seed))
    theta = rng.normal(0.3, 0.03, n)
    in_field = np.stack([np.cos(theta), np.sin(theta), rng.normal(W * RES / 2, 0.15, n), rng.normal(H * RES / 2, 0.15, n)], axis=1)
    return compose(origin, in_field), rng.uniform(0.5, 1.5, n)


def scan(B, seed=9):
    rng = np.random.Generator(np.random.MT19937(seed))
    angle, r = np.linspace(-2.3, 2.3, B), rng.uniform(0.3, 1.8, B)
    return np.stack([r * np.cos(angle), r * np.sin(angle)], axis=1)


_filters = {}


def filter_for(prob):
    if prob not in _filters:
        _filters[prob] = Amcl(grid_at(ORIGIN), MOTION, LF_PROB if prob else LF, AmclParams(min_particles=1024, max_particles=1024), seed=11)
    return _filters[prob]


@pytest.fixture(scope="module", autouse=True)
def _close_filters():
    yield
    for f in _filters.values():
        f.close()
    _filters.clear()


def reweighted(f, arm, states, w0, points, moved):
    """The weights after one reweight of (states, w0) under `arm`; the counters that moved and the rebuilds are checked."""
    f.set_option("lf_pose_ahead", arm)
    f.set_particles(states, w0)
    before = {c: f.counter(c) for c in COUNTERS + ("field_pose_rebuilds",)}
    f.reweight(points)
    delta = {c: f.counter(c) - before[c] for c in before}
    assert delta == {**{c: (1 if c in moved else 0) for c in COUNTERS}, "field_pose_rebuilds": arm}, (arm, delta)
    return f.particles()[1]


def check_form(form, prob):
    n, options, moved, kind = FORMS[form]
    f = filter_for(prob)
    for name, value in {**DEFAULTS, **options}.items():
        f.set_option(name, value)
    f.set_likelihood_field(field(kind))
    states, w0 = cloud(n)
    for B in BEAMS:
        points = scan(B)
        # (a launch in segments - 264 beams, fewer than 4096 waves - is never the queue's)
        moved_here = tuple(c for c in moved if not (c == "lf_queue_launches" and B >= 128))
        form_itself = reweighted(f, 0, states, w0, points, moved_here)
        loaded = reweighted(f, 1, states, w0, points, moved_here)
        assert np.all(np.isfinite(form_itself)) and not np.array_equal(form_itself, w0)
        assert np.array_equal(loaded, form_itself), (form, B, int(np.sum(loaded != form_itself)))


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_form_gives_the_same_bits_with_the_poses_loaded(form):
    check_form(form, prob=False)


@pytest.mark.parametrize("form", PROB_FORMS)
def test_the_prob_models_instances_too(form):
    check_form(form, prob=True)


# ---- the sequences: what sets the fact and what voids it --------------------------------------------------------------------------------
SEQ_OPTIONS = {"lf_small_particles": 512, "sort_min_particles": 512, "lf_patch": 2, "lf_queue_grid": 2}  # the patch kernel's queue form
CONTROL = (se2_from_xytheta(0.3, 0.0, 0.02), se2_from_xytheta(0.0, 0.0, 0.0))
POINTS = scan(9)


def make(arm, grid=None, n=N_PATCH, options=SEQ_OPTIONS, seed=21):
    return Amcl(grid or grid_at(ORIGIN), MOTION, LF, AmclParams(min_particles=n, max_particles=n), seed=seed,
                options={**options, "lf_pose_ahead": arm})


def fresh_twin(f, w_before, reweights, grid=None):
    """A fresh context given f's states and the weights f had before its `reweights` reweights: what it makes of them."""
    g = make(1, grid)
    g.set_particles(f.particles()[0], w_before)
    for _ in range(reweights):
        g.reweight(POINTS)
    assert g.counter("field_pose_rebuilds") == 1
    w = g.particles()[1]
    g.close()
    return w


def run_arms(sequence, reweights=1, grid_after=None):
    """sequence(f) -> the weights before the reweights it ends with; both arms and the fresh twin; returns the load arm's rebuilds."""
    out = []
    for arm in (0, 1):
        f = make(arm)
        f.set_particles(*cloud(N_PATCH))
        w_before = sequence(f)
        out.append((f.particles(), f.counter("field_pose_rebuilds"), fresh_twin(f, w_before, reweights, grid_after) if arm else None))
        f.close()
    (s0, w0), r0, _ = out[0]
    (s1, w1), r1, twin = out[1]
    assert r0 == 0
    assert np.array_equal(s0, s1) and np.array_equal(w0, w1) and np.array_equal(w1, twin)
    return r1


def test_propagate_reweight_reweight_reuses_what_the_propagation_wrote():
    def sequence(f):
        f.propagate(*CONTROL, 1)
        w = f.particles()[1]
        f.reweight(POINTS)
        f.reweight(POINTS)
        return w
    assert run_arms(sequence, reweights=2) == 0


def test_resample_then_reweight_rebuilds_once():
    def sequence(f):
        f.propagate(*CONTROL, 1)
        f.reweight(POINTS)
        f.normalize()
        f.resample(0.0, 1)
        w = f.particles()[1]
        f.reweight(POINTS)
        f.reweight(POINTS)
        return w
    assert run_arms(sequence, reweights=2) == 1


def test_set_particles_then_reweight_rebuilds_once():
    def sequence(f):
        f.propagate(*CONTROL, 1)
        f.reweight(POINTS)
        states, w = cloud(N_PATCH, seed=6)
        f.set_particles(states, w)
        f.reweight(POINTS)
        return w
    assert run_arms(sequence) == 1


@pytest.mark.parametrize("swap", ["update_map", "update_map_async", "use_map", "set_likelihood_field"])
def test_a_map_given_behind_the_propagation_voids_what_it_wrote(swap):
    """The propagation stored the poses in the OLD map's frame; the reweight reads the new one's."""
    grid2 = grid_at(ORIGIN_2)
    shared = SharedMap(grid2, LF) if swap == "use_map" else None

    def sequence(f):
        f.propagate(*CONTROL, 1)
        if swap == "update_map":
            f.update_map(grid2)
        elif swap == "update_map_async":
            f.update_map_async(grid2)
            f.map_commit(wait=True)
        elif swap == "use_map":
            f.use_map(shared)
        else:
            f.set_likelihood_field(field("palette"))
        w = f.particles()[1]
        f.reweight(POINTS)
        return w
    twin_grid = grid_at(ORIGIN) if swap == "set_likelihood_field" else grid2
    if swap == "set_likelihood_field":  # (the twin needs the same field: it is given one the same way)
        rebuilds = []
        for arm in (0, 1):
            f = make(arm)
            f.set_particles(*cloud(N_PATCH))
            sequence(f)
            rebuilds.append((f.particles()[1], f.counter("field_pose_rebuilds")))
            f.close()
        assert np.array_equal(rebuilds[0][0], rebuilds[1][0]) and [r[1] for r in rebuilds] == [0, 1]
    else:
        assert run_arms(sequence, grid_after=twin_grid) == 1
    if shared is not None:
        shared.close()


@pytest.mark.parametrize("options,n", [
    ({"lf_small_particles": 512, "sort_min_particles": 512, "lf_patch": 2, "lf_queue_grid": 2, "small_fused": 0}, N_PATCH),  # k_propagate<true>
    ({}, N_WAVE),                                  # the small cycle: k_propagate_small, k_reweight_lf_beams, k_small_tail
    ({"lf_variant": 1, "noise_ahead": 0}, 66_000),  # k_propagate<false>, the index-order kernel
])
def test_the_steady_cycle_never_rebuilds_and_keeps_its_bits(options, n):
    results = []
    for arm in (0, 1):
        f = make(arm, n=n, options=options)
        f.initialize((3.0, 1.0, 0.7), np.diag([0.02, 0.02, 0.001]))
        estimates = [f.update(se2_from_xytheta(0.3 * k, 0.0, 0.02 * k), POINTS) for k in range(1, 5)]
        assert all(e is not None for e in estimates) and f.last_info["resampled"]
        results.append((estimates, f.particles(), f.counter("field_pose_rebuilds")))
        f.close()
    (e0, p0, r0), (e1, p1, r1) = results
    assert (r0, r1) == (0, 0)
    for a, b in zip(e0, e1):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1], p1[1])


def test_a_fused_batch_member_equals_its_lone_twin_in_both_arms():
    params = AmclParams(min_particles=600, max_particles=600, resample_interval=1000)
    mean, cov = (3.0, 1.0, 0.7), np.diag([0.02, 0.02, 0.001])
    seen = []
    for arm in (0, 1):
        batch = AmclBatch([dict(grid=grid_at(ORIGIN), motion=MOTION, sensor=LF, params=params, seed=31, options={"lf_pose_ahead": arm})])
        twin = Amcl(grid_at(ORIGIN), MOTION, LF, params, seed=31, options={"lf_pose_ahead": arm})
        for f in batch.members + [twin]:
            f.initialize(mean, cov)
        for k in range(1, 3):
            control = se2_from_xytheta(0.3 * k, 0.0, 0.02 * k)
            got = batch.update([control], [POINTS])
            want = twin.update(control, POINTS)
            assert np.array_equal(got[0][0], want[0]) and np.array_equal(got[0][1], want[1])
        assert batch.counter("members_fused") == 2  # (one member, two cycles)
        member = batch.members[0].particles()
        assert np.array_equal(member[0], twin.particles()[0]) and np.array_equal(member[1], twin.particles()[1])
        assert batch.members[0].counter("field_pose_rebuilds") == 0 and twin.counter("field_pose_rebuilds") == 0
        seen.append(member)
        batch.close()
        twin.close()
    assert np.array_equal(seen[0][0], seen[1][0]) and np.array_equal(seen[0][1], seen[1][1])
