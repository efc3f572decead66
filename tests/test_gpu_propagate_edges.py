"""The propagation kernels (k_propagate_small, k_propagate<false>) against an extended-precision restatement, at the edges.

test_gpu_parity.py holds a propagated set to the double-precision oracle on one mild control action.  Here the kernels' own arithmetic
(kernels.hip: sincos_fast, rot_from_complex_fast, rot_mul_fast, pose_mul_fast, box_muller_fast) is held to
tests/propagate_reference.py - the same motion models in extended precision - in conditioned units (that file's docstring), on the
sampler the kernel itself received (Amcl.last_sampler, bit for bit), at every size where the launch geometry changes, and on arguments
chosen for the helpers: angles at the quadrant boundaries of the sine / cosine reduction, rotations that are not unit, standard
deviations that send the angles through a hundred thousand quadrants and past the library fallback at 1e6.

The limit everywhere is max(4, 4 * oracle_worst) units, oracle_worst being the double-precision oracle's worst error on the same rows
against the same reference (test_propagate_reference_cpu.py holds it to 4 without a GPU); it is never taken from the device.  DESIGN.md,
"The propagation's own forms", has the measured figures and the mutants these tests were shown to catch.
"""
import numpy as np
import pytest

import propagate_families as fam
from beluga_amd.amcl import (Amcl, AmclParams, DifferentialDriveModelParam, OmnidirectionalDriveModelParam, StationaryModelParam)
from oracle import binding as orc
from test_gpu_parity import LF, rooms_grid

pytestmark = pytest.mark.gpu

KIND_ID = {"differential": 0, "omnidirectional": 1, "stationary": 2}


def motion_param(kind, alphas):
    if kind == "differential":
        return DifferentialDriveModelParam(*alphas[:4])
    if kind == "omnidirectional":
        return OmnidirectionalDriveModelParam(*alphas[:5])
    return StationaryModelParam()


@pytest.fixture(scope="module")
def filters():
    """One filter per motion model and noise setting, made on first use and kept for the module (a filter builds a likelihood field)."""
    made = {}
    grid = rooms_grid(64, 1)

    def get(kind, alphas=None, capacity=fam.N_MAX):
        alphas = fam.ALPHAS[kind] if alphas is None else alphas
        key = (kind, tuple(alphas), capacity)
        if key not in made:
            made[key] = Amcl(grid, motion_param(kind, alphas), LF, AmclParams(min_particles=capacity, max_particles=capacity), seed=fam.SEED)
        return made[key]

    yield get
    for f in made.values():
        f.close()


def run(f, states, control, step):
    """-> (the propagated states, the sampler the kernel received)"""
    f.set_particles(states, np.ones(len(states)))
    f.propagate(control[0], control[1], step=step)
    got = f.particles()[0]
    assert got.shape == (len(states), 4)
    return got, f.last_sampler()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_last_sampler_is_refused_before_a_propagation_and_read_only_after():
    from beluga_amd import capi
    f = Amcl(rooms_grid(64, 1), motion_param("differential", fam.ALPHAS["differential"]), LF, AmclParams(min_particles=64, max_particles=64),
             seed=fam.SEED)
    with pytest.raises(capi.MclError):
        f.last_sampler()
    states = fam.shape_states(64)
    got, sampler = run(f, states, (fam.SHAPE_POSE, fam.SHAPE_PREV), 7)
    assert np.array_equal(bits(f.last_sampler()), bits(sampler)) and np.array_equal(bits(f.particles()[0]), bits(got))
    assert sampler[6] == 0 and sampler[2] == pytest.approx(np.hypot(0.3, 0.1), rel=1e-14)
    f.close()


@pytest.mark.parametrize("n", fam.N_SMALL + fam.N_CHUNKED)
@pytest.mark.parametrize("kind", fam.KINDS)
def test_shapes_both_kernels_every_model(filters, kind, n):
    """n up to 65 536: k_propagate_small; above: k_propagate<false>, 33 chunks of 2048 and their neighbours.  Steps 0, 7, 2^32 - 1."""
    f = filters(kind)
    all_states = fam.shape_states(fam.N_MAX)
    control = (fam.SHAPE_POSE, fam.SHAPE_PREV)
    rows = fam.compared_rows(n)
    own = orc.motion_sampler(kind, *control, fam.ALPHAS[kind])
    for step in fam.STEPS:
        got, sampler = run(f, all_states[:n], control, step)
        assert sampler[6] == KIND_ID[kind]
        # (wiring only - what make_sampler is held to: test_cycle_host_cpu.py; the reference below runs on `sampler` itself.  Only the
        # fields the model reads: the stationary model reads none, the differential one not the rotation to the direction of travel
        # (first_c, first_s), and the two sides leave different things in those.)
        read = {"differential": 7, "omnidirectional": 9, "stationary": 0}[kind]
        np.testing.assert_allclose(sampler[:read], own[:read], rtol=1e-12, atol=1e-15)
        reference, oracle_errors = fam.yardstick(kind, "shape", all_states, sampler, control, fam.ALPHAS[kind], step)
        fam.hold(f"{kind} n={n} step={step}", got[rows], fam.take(reference, rows), (oracle_errors[0][rows], oracle_errors[1][rows]))


@pytest.mark.parametrize("kind", fam.KINDS)
def test_same_bits_across_the_two_kernels(filters, kind):
    """kernels.hip: "same expressions: same bits" - the first 65 536 rows of a run of 65 537 (k_propagate<false>) are those of a run of
    65 536 (k_propagate_small) on the same states, seed and step.  With the sampled comparison above this covers every row."""
    f = filters(kind)
    states = fam.shape_states(fam.SMALL_MAX + 1)
    control = (fam.SHAPE_POSE, fam.SHAPE_PREV)
    small, _ = run(f, states[:fam.SMALL_MAX], control, 7)
    chunked, _ = run(f, states, control, 7)
    assert np.array_equal(bits(chunked[:fam.SMALL_MAX]), bits(small))
    assert not np.array_equal(bits(chunked[fam.SMALL_MAX]), bits(states[fam.SMALL_MAX]))  # (the last row moved too)


@pytest.mark.parametrize("n", [1, 255, 257, 2049])
def test_no_write_past_n(filters, n):
    """mcl_set_num_particles keeps the rows (it changes the count alone): N rows loaded, n of them propagated, N restored - rows
    n .. N - 1 are bit-unchanged, rows 0 .. n - 1 are what a run of all N rows makes of them."""
    N = 4096
    f = filters("differential")
    states = fam.shape_states(N)
    control = (fam.SHAPE_POSE, fam.SHAPE_PREV)
    whole, _ = run(f, states, control, 7)
    f.set_particles(states, np.ones(N))
    f.set_num_particles(n)
    f.propagate(control[0], control[1], step=7)
    assert f.num_particles() == n
    f.set_num_particles(N)
    after = f.particles()[0]
    assert np.array_equal(bits(after[n:]), bits(states[n:]))
    assert np.array_equal(bits(after[:n]), bits(whole[:n]))


def test_angle_edges_noise_free(filters):
    """All alphas 0, so the sine / cosine see the sampler's m1 and m2 as they are: each next to 0, +-pi/4, +-pi/2, +-3pi/4, +-pi, and
    +-1e-9, +-1e-300.  256 states: headings from the same list, half with rotations scaled by 1 +- 2^-30 (rot_mul_fast's n2 != 1
    branch), positions 0, +-1e-3, +-1e6."""
    zero = (0.0,) * 4
    f = filters("differential", zero, 256)
    states = fam.edge_states()
    realised, worst = [], (0.0, 0.0)
    for j, control in enumerate(fam.edge_controls()):
        got, sampler = run(f, states, control, j)
        assert sampler[1] == 0.0 and sampler[3] == 0.0 and sampler[5] == 0.0 and sampler[6] == 0
        realised += [sampler[0], sampler[4]]
        reference, oracle_errors = fam.yardstick("differential", "edge", states, sampler, control, zero, j)
        figures = fam.hold(f"edge {j} m1={sampler[0]!r} m2={sampler[4]!r}", got, reference, oracle_errors)
        worst = tuple(max(a, b) for a, b in zip(worst, figures))
    print(f"edges: worst rotation {worst[0]:.3f}, position {worst[1]:.3f} units")
    fam.assert_edges_reached(realised)


@pytest.mark.parametrize("kind", fam.FAR_KINDS)
def test_rotations_far_from_unit(filters, kind):
    """Input rotations of length 1e-3 .. 1e3: rot_from_complex_fast's reciprocal square root on arguments that are not 1 to a few ulp
    (everywhere else they are: a sine / cosine pair, or a product after rot_mul_fast's first-order renormalisation)."""
    f = filters(kind)
    states = fam.far_from_unit_states()
    control = (fam.SHAPE_POSE, fam.SHAPE_PREV)
    got, sampler = run(f, states, control, 7)
    reference, oracle_errors = fam.yardstick(kind, "far", states, sampler, control, fam.ALPHAS[kind], 7)
    fam.hold(f"far from unit, {kind}", got, reference, oracle_errors)


@pytest.mark.parametrize("n", [fam.WIDE_N_SMALL, fam.WIDE_N_CHUNKED])
def test_wide_angles(filters, n):
    """alpha2 = alpha3 = 9 over a translation of 1e5: standard deviations of 3e5 radians - k of the reduction up to +-600 000, both
    signs, every k mod 4, and the library fallback beyond 1e6 (about 1 particle in 600).  Every sampler field is exact in double."""
    f = filters("differential", fam.WIDE_ALPHAS, fam.WIDE_N_CHUNKED)
    states = fam.wide_states(n)
    control = (fam.WIDE_POSE, fam.WIDE_PREV)
    got, sampler = run(f, states, control, fam.WIDE_STEP)
    assert np.array_equal(sampler, np.array(fam.WIDE_SAMPLER + (0.0, 1.0, 0.0))), sampler  # (values: a zero of either sign adds alike)
    assert np.array_equal(bits(sampler[[1, 2, 3, 5]]), bits(np.array([3e5, 1e5, 3e5, 3e5])))
    rows = fam.compared_rows(n) if n > fam.SMALL_MAX else np.arange(n)
    reference, oracle_errors = fam.yardstick("differential", f"wide{n}", states, sampler, control, fam.WIDE_ALPHAS, fam.WIDE_STEP)
    fam.assert_wide_reached(reference.angles[rows])
    fam.hold(f"wide n={n}", got[rows], fam.take(reference, rows), (oracle_errors[0][rows], oracle_errors[1][rows]))


def test_in_place_rotation_branch(filters):
    """A translation of at most distance_threshold = 0.01 has no direction: the first rotation is the identity, the second the whole turn."""
    f = filters("differential")
    states = fam.shape_states(4096)
    for k, pose in enumerate(fam.IN_PLACE_POSES):
        control = (pose, fam.SHAPE_PREV)
        got, sampler = run(f, states, control, 8)
        assert sampler[0] == 0.0 and sampler[7] == 1.0 and sampler[8] == 0.0
        reference, oracle_errors = fam.yardstick("differential", "shape", states, sampler, control, fam.ALPHAS["differential"], 8)
        fam.hold(f"in place {k}", got, reference, oracle_errors)
