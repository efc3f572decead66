"""The extended-precision restatement of the propagation (propagate_reference.py) against the double-precision oracle, on every input
family of test_gpu_propagate_edges.py - no GPU.

The oracle is the reference project's arithmetic in double (library sin / cos / hypot, divisions); it must stay within 4 conditioned
units of the restatement everywhere.  That keeps the restatement and the unit honest - a unit that is too small, or a motion model
restated wrongly, shows here - and it is the yardstick the GPU tests take their limit from.  What each family is there to reach (the
library fallback, large and negative quadrant indices, both sides of every quadrant boundary) is asserted on the restatement alone.
"""
import math

import numpy as np
import pytest

import propagate_families as fam
import propagate_reference as ref
from oracle import binding as orc

ORACLE_LIMIT = 4.0


def test_philox_words_and_uniforms_are_the_oracles():
    """The integer part, word for word: indices below and above 2^32, every step of the shapes family, both purposes."""
    rng = np.random.Generator(np.random.PCG64(1))
    index = np.concatenate([np.arange(70), rng.integers(0, 2 ** 32, 40), rng.integers(2 ** 32, 2 ** 40, 40)]).astype(np.uint64)
    for seed in (fam.SEED, 0, 2 ** 63 + 12345):
        for step in fam.STEPS:
            for purpose in (0, 1):
                got = ref.draw(seed, step, purpose, index)
                want = np.stack([orc.draw(seed, step, purpose, int(i)) for i in index])
                assert np.array_equal(got, want), (seed, step, purpose)
    assert ref.uniform53(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53
    assert ref.uniform53(0, 0x7FF) == 0.0 and ref.uniform53(0, 0x800) == 2.0 ** -53


def test_extended_precision_is_what_the_docstring_says():
    if ref.USE_MPMATH:
        import mpmath
        assert mpmath.mp.prec >= 64
    else:
        assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    one = ref.ext(np.array([1.0]))
    assert ref.to_f64((one + ref.ext(np.array([2.0 ** -60]))) - one)[0] == 2.0 ** -60  # lost in double, kept here


@pytest.mark.parametrize("step", fam.STEPS)
@pytest.mark.parametrize("kind", fam.KINDS)
def test_oracle_within_4_units_on_the_shapes_family(kind, step):
    states = fam.shape_states(fam.N_MAX)
    control = (fam.SHAPE_POSE, fam.SHAPE_PREV)
    sampler = orc.motion_sampler(kind, *control, fam.ALPHAS[kind])
    r, errors = fam.yardstick(kind, "shape", states, sampler, control, fam.ALPHAS[kind], step)
    print(f"{kind} step {step}: oracle rotation {errors[0].max():.3f}, position {errors[1].max():.3f} units")
    assert errors[0].max() <= ORACLE_LIMIT and errors[1].max() <= ORACLE_LIMIT
    # (the rows a GPU case compares are among them, and none is empty)
    for n in fam.N_SMALL + fam.N_CHUNKED:
        rows = fam.compared_rows(n)
        assert len(rows) and rows.min() >= 0 and rows.max() == n - 1 and len(np.unique(rows)) == len(rows)


def test_compared_rows_hold_both_ends_of_every_chunk():
    for n in fam.N_CHUNKED:
        rows = set(fam.compared_rows(n).tolist())
        for first in range(0, n, fam.CHUNK):
            end = min(first + fam.CHUNK, n)
            assert first in rows and end - 1 in rows
            assert all(i in rows for i in range(first, min(first + 64, end))) and all(i in rows for i in range(max(first, end - 64), end))
        assert len(rows) >= 2048


def test_oracle_within_4_units_on_the_in_place_rotation_branch():
    states = fam.shape_states(4096)
    for k, pose in enumerate(fam.IN_PLACE_POSES):
        d = math.hypot(pose[2] - fam.SHAPE_PREV[2], pose[3] - fam.SHAPE_PREV[3])
        assert d <= 0.01
        sampler = orc.motion_sampler("differential", pose, fam.SHAPE_PREV, fam.ALPHAS["differential"])
        assert sampler[0] == 0.0  # the first rotation is the identity: the translation is not long enough to have a direction
        r, errors = fam.yardstick("differential", "shape", states, sampler, (pose, fam.SHAPE_PREV), fam.ALPHAS["differential"], 8)
        print(f"in place {k}: oracle rotation {errors[0].max():.3f}, position {errors[1].max():.3f} units")
        assert errors[0].max() <= ORACLE_LIMIT and errors[1].max() <= ORACLE_LIMIT


@pytest.mark.parametrize("kind", fam.FAR_KINDS)
def test_oracle_within_4_units_on_rotations_far_from_unit(kind):
    states = fam.far_from_unit_states()
    length = np.hypot(states[:, 0], states[:, 1])
    assert (np.abs(length - 1.0) > 0.2).all() and length.min() < 2e-3 and length.max() > 500
    control = (fam.SHAPE_POSE, fam.SHAPE_PREV)
    sampler = orc.motion_sampler(kind, *control, fam.ALPHAS[kind])
    r, errors = fam.yardstick(kind, "far", states, sampler, control, fam.ALPHAS[kind], 7)
    print(f"far from unit, {kind}: oracle rotation {errors[0].max():.3f}, position {errors[1].max():.3f} units")
    assert errors[0].max() <= ORACLE_LIMIT and errors[1].max() <= ORACLE_LIMIT


def test_wide_family_reaches_the_fallback_and_every_quadrant():
    sampler = orc.motion_sampler("differential", fam.WIDE_POSE, fam.WIDE_PREV, fam.WIDE_ALPHAS)
    assert np.array_equal(sampler[:6], np.array(fam.WIDE_SAMPLER)), sampler  # exact in double: the same bits from any correct sampler
    for n in (fam.WIDE_N_SMALL, fam.WIDE_N_CHUNKED):
        states = fam.wide_states(n)
        r, errors = fam.yardstick("differential", f"wide{n}", states, sampler, (fam.WIDE_POSE, fam.WIDE_PREV), fam.WIDE_ALPHAS, fam.WIDE_STEP)
        rows = fam.compared_rows(n) if n > fam.SMALL_MAX else np.arange(n)
        print(f"wide n={n}: oracle rotation {errors[0][rows].max():.3f}, position {errors[1][rows].max():.3f} units")
        assert errors[0][rows].max() <= ORACLE_LIMIT and errors[1][rows].max() <= ORACLE_LIMIT
        fam.assert_wide_reached(r.angles[rows])


def test_edge_family_lands_on_both_sides_of_every_boundary():
    """(what "both sides" means: propagate_families.assert_edges_reached)"""
    realised = []
    zero = (0.0,) * 4
    states = fam.edge_states()
    worst_rot = worst_pos = 0.0
    for j, (pose, prev) in enumerate(fam.edge_controls()):
        sampler = orc.motion_sampler("differential", pose, prev, zero)
        assert sampler[1] == 0.0 and sampler[3] == 0.0 and sampler[5] == 0.0 and sampler[2] == pytest.approx(fam.EDGE_T, rel=1e-15)
        realised += [sampler[0], sampler[4]]
        r, errors = fam.yardstick("differential", "edge", states, sampler, (pose, prev), zero, j)
        worst_rot, worst_pos = max(worst_rot, errors[0].max()), max(worst_pos, errors[1].max())
    print(f"edges: oracle rotation {worst_rot:.3f}, position {worst_pos:.3f} units")
    assert worst_rot <= ORACLE_LIMIT and worst_pos <= ORACLE_LIMIT
    fam.assert_edges_reached(realised)
    # the states: both kinds of rotation, and every place
    n2 = states[:, 0] ** 2 + states[:, 1] ** 2
    assert (np.abs(n2[:128] - 1.0) <= 2.0 ** -52).all() and (np.abs(n2[128:] - 1.0) > 2.0 ** -31).all()
    assert (n2[128:] > 1.0).any() and (n2[128:] < 1.0).any()
    assert set(np.unique(states[:, 2]).tolist()) == set(np.unique(states[:, 3]).tolist()) == {0.0, 1e-3, -1e-3, 1e6, -1e6}
