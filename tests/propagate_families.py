"""The inputs of the propagation tests, shared by test_propagate_reference_cpu.py (reference against oracle, and what each family
must reach) and test_gpu_propagate_edges.py (device against reference).  Plain numpy and the oracle; nothing of the code under test."""
import math

import numpy as np

import propagate_reference as ref
from oracle import binding as orc

SEED = 11
CHUNK = 2048  # kChunk (kernels.h): k_propagate's workgroup
SMALL_MAX = 65_536  # launch_propagate: k_propagate_small up to here, k_propagate<false> above
N_SMALL = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 65_536)
N_CHUNKED = (65_537, 67_583, 67_584, 67_585)  # 33 chunks of 2048 and their neighbours
N_MAX = max(N_CHUNKED)
STEPS = (0, 7, 2 ** 32 - 1)
KINDS = ("differential", "omnidirectional", "stationary")
ALPHAS = {"differential": (0.1, 0.05, 0.1, 0.05), "omnidirectional": (0.1, 0.05, 0.1, 0.05, 0.08), "stationary": (0.0,) * 5}


def pose(x, y, theta):
    """(cos, sin, x, y), the rotation normalised as SO2's constructor does."""
    c, s = math.cos(theta), math.sin(theta)
    length = math.hypot(c, s)
    return np.array([c / length, s / length, x, y])


# ---- shapes ------------------------------------------------------------------------------------------------
SHAPE_POSE, SHAPE_PREV = pose(1.3, 0.4, 0.35), pose(1.0, 0.3, 0.30)  # (test_gpu_parity.py's control action)
IN_PLACE_POSES = (pose(1.0, 0.3, 0.9), pose(1.004, 0.297, -2.0))  # from SHAPE_PREV: distances 0 and 0.005, both <= distance_threshold

_shape_states = None


def shape_states(n):
    """The first n of N_MAX seeded states: headings over the whole circle, positions of a few metres.  (One array, so that a row's
    reference does not depend on n.)"""
    global _shape_states
    if _shape_states is None:
        rng = np.random.Generator(np.random.PCG64(20))
        h = rng.uniform(-math.pi, math.pi, N_MAX)
        c, s = np.cos(h), np.sin(h)
        length = np.hypot(c, s)
        _shape_states = np.stack([c / length, s / length, rng.normal(0.0, 3.0, N_MAX), rng.normal(0.0, 3.0, N_MAX)], axis=1)
        _shape_states.setflags(write=False)
    return _shape_states[:n]


def compared_rows(n):
    """Every row up to 4096 particles; above, the first and last 64 rows of every 2048-chunk (the last chunk ends at n) and 2048
    seeded random rows."""
    if n <= 4096:
        return np.arange(n)
    rows = [np.random.Generator(np.random.PCG64(n)).integers(0, n, 2048)]
    for first in range(0, n, CHUNK):
        end = min(first + CHUNK, n)
        rows.append(np.arange(first, min(first + 64, end)))
        rows.append(np.arange(max(end - 64, first), end))
    return np.unique(np.concatenate(rows))


# ---- angle edges, noise-free -----------------------------------------------------------------------------------
EDGE_T = 2.0
EDGE_BOUNDARIES = tuple(k * math.pi / 4 for k in range(-4, 5))  # 0, +-pi/4, +-pi/2, +-3pi/4, +-pi: the doubles nearest


def edge_angles():
    """The double nearest each boundary and 4 nextafter steps either way, then +-1e-9 and +-1e-300: 85 angles."""
    out = []
    for b in EDGE_BOUNDARIES:
        below, above = [b], [b]
        for _ in range(4):
            below.append(math.nextafter(below[-1], -math.inf))
            above.append(math.nextafter(above[-1], math.inf))
        out += below[:0:-1] + [b] + above[1:]
    return out + [1e-9, -1e-9, 1e-300, -1e-300]


def edge_controls():
    """One control action per angle of the list: prev at the origin with heading 0, pose = (T cos phi, T sin phi, psi); phi takes the
    list in order and psi - phi takes it in another order (a stride coprime to its length), so each sweeps all of it."""
    angles = edge_angles()
    m = len(angles)
    prev = pose(0.0, 0.0, 0.0)
    out = []
    for j, phi in enumerate(angles):
        psi = phi + angles[(37 * j + 11) % m]
        p = pose(EDGE_T * math.cos(phi), EDGE_T * math.sin(phi), psi)
        out.append((p, prev))
    return out


def edge_states(n=256):
    """Headings from the list; the first half's rotations are unit to rounding, the second half's are scaled by 1 +- 2^-30 (rot_mul's
    n2 != 1 branch for certain); positions take 0, +-1e-3, +-1e6."""
    angles = edge_angles()
    places = (0.0, 1e-3, -1e-3, 1e6, -1e6)
    s = np.empty((n, 4))
    for i in range(n):
        s[i] = pose(places[i % 5], places[(i // 5) % 5], angles[(i * 7) % len(angles)])
        if i >= n // 2:
            s[i, :2] *= 1.0 + (2.0 ** -30 if i % 2 else -(2.0 ** -30))
    return s


FAR_SCALES = (0.5, 0.75, 1.5, 3.0, 1e-3, 1e3)
# (not the stationary model: its one product turns the drawn step by the rotation AS STORED, so a length of 1e3 scales the step itself
# - the unit is worked out for steps of the size drawn; its rotation goes through the same helpers as the other two models')
FAR_KINDS = ("differential", "omnidirectional")


def far_from_unit_states(n=2048):
    """The shapes family's states with their rotations scaled well away from unit length: the one place where the normalisation
    z * rsqrt(|z|^2) gets an argument that is not 1 to a few ulp, so where the accuracy of the reciprocal square root itself - the
    hardware's estimate and its two Newton steps - shows in the result (the shared form divides by hypot, whatever the length)."""
    s = shape_states(n).copy()
    s[:, :2] *= np.array(FAR_SCALES)[np.arange(n) % len(FAR_SCALES)][:, None]
    return s


def assert_edges_reached(realised):
    """The REALISED angles of the edge family - m1 and m2 of each control action's sampler, which the noise-free model hands to the
    sine / cosine as they are - against each boundary k pi/4 in extended precision: some within a few ulp below it and some above.
    (+-pi: atan2 wraps, so "beyond pi" is just above -pi; the two ends are each approached from inside.)"""
    realised = np.asarray(realised, dtype=np.float64)
    pi = ref.x_atan2(ref.ext(np.array([0.0])), ref.ext(np.array([-1.0])))[0]  # pi to extended precision
    for k in range(-3, 4):
        diff = ref.to_f64(ref.ext(realised) - pi * k / 4)
        near = np.abs(diff) < 1e-14
        assert (diff[near] < 0).any() and (diff[near] > 0).any(), (k, np.sort(diff[near]))
    assert ((realised > 0) & (np.abs(realised - math.pi) < 1e-14)).any() and ((realised < 0) & (np.abs(realised + math.pi) < 1e-14)).any()
    assert (np.abs(np.abs(realised) - 1e-9) < 1e-24).any()
    assert ((realised != 0.0) & (np.abs(realised) < 1e-299)).any()


def assert_wide_reached(angles):
    """The wide family's arguments of the sine / cosine: the library fallback, the fast path, a large k, and every k mod 4 for both signs."""
    theta = np.asarray(angles, dtype=np.float64).reshape(-1)
    beyond = np.abs(theta) >= ref.FALLBACK
    assert beyond.sum() >= 10, beyond.sum()
    assert (~beyond).sum() >= 1000
    k = ref.quadrant(theta[~beyond])
    assert np.abs(k).max() > 100_000
    for sign in (1, -1):
        residues = set((k[k * sign > 0] % 4).tolist())
        assert residues == {0, 1, 2, 3}, (sign, residues)


# ---- wide angles -------------------------------------------------------------------------------------------
WIDE_ALPHAS = (0.0, 9.0, 9.0, 0.0)
WIDE_POSE, WIDE_PREV = np.array([1.0, 0.0, 1e5, 0.0]), np.array([1.0, 0.0, 0.0, 0.0])
WIDE_SAMPLER = (0.0, 3e5, 1e5, 3e5, 0.0, 3e5)  # every field exact in double
WIDE_N_SMALL, WIDE_N_CHUNKED = 20_000, 70_000
WIDE_STEP = 7


def wide_states(n):
    rng = np.random.Generator(np.random.PCG64(21))
    h = rng.uniform(-math.pi, math.pi, n)
    c, s = np.cos(h), np.sin(h)
    length = np.hypot(c, s)
    return np.stack([c / length, s / length, rng.normal(0.0, 3.0, n), rng.normal(0.0, 3.0, n)], axis=1)


# ---- holding a result to the reference ------------------------------------------------------------------------
def take(r, rows):
    return ref.Reference(*(a[rows] for a in r))


_yardsticks = {}


def yardstick(kind, key, states, sampler, control, alphas, step, seed=SEED):
    """-> (the reference of every row of `states` on `sampler`, the double-precision oracle's error per row as (rotation, position)
    in units).  The oracle's differential model runs on `sampler` itself; for the other two it builds its own from the control action
    (pose, prev), and its error is taken against the reference on THAT sampler.  Computed once per case (`key` names `states`)."""
    sampler = np.asarray(sampler, dtype=np.float64)
    k = (kind, key, len(states), sampler.tobytes(), step, seed)
    if k not in _yardsticks:
        r = ref.propagate(states, sampler, seed, step)
        if kind == "differential":
            oracle_errors = ref.errors(r, orc.propagate(states, sampler[:6], seed=seed, step=step))
        else:
            own = orc.motion_sampler(kind, control[0], control[1], alphas)
            r_own = r if np.array_equal(own, sampler) else ref.propagate(states, own, seed, step)
            oracle_errors = ref.errors(r_own, orc.propagate_kind(states, kind, control[0], control[1], alphas, seed=seed, step=step))
        _yardsticks[k] = (r, oracle_errors)
    return _yardsticks[k]


def hold(label, got, reference, oracle_errors):
    """Asserts `got` within limit(the oracle's worst on the same rows) units of `reference`, rotation and position each; prints the
    figures first.  -> the figures."""
    rot, pos = ref.worst(reference, got)
    oracle_rot, oracle_pos = (float(e.max()) if len(e) else 0.0 for e in oracle_errors)
    lim_rot, lim_pos = ref.limit(oracle_rot), ref.limit(oracle_pos)
    print(f"{label}: rotation {rot:.3f} (oracle {oracle_rot:.3f}, limit {lim_rot:.2f}), "
          f"position {pos:.3f} (oracle {oracle_pos:.3f}, limit {lim_pos:.2f}) units")
    assert math.isfinite(oracle_rot) and math.isfinite(oracle_pos), label
    assert rot <= lim_rot, f"{label}: rotation {rot} units > {lim_rot}"
    assert pos <= lim_pos, f"{label}: position {pos} units > {lim_pos}"
    return rot, pos
