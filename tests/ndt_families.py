"""Inputs shared by tests/test_ndt_reference_cpu.py and tests/test_gpu_ndt_edges.py: NDT maps, poses and measurement cells ENGINEERED to
sit where the reweight kernels' cell choice can go wrong.  Deterministic (found by search at import); no device.

A family is a function returning a list of Case: a map (keys, means, covariances, resolution), a neighbour kernel and the model's
parameters, states [m, 4], measurement cells (means [K, 2], covariances [K, 2, 2]) that go through reweight_ndt_cells in this order,
prior weights that are not 1, and `pairs`: the engineered (state, cell) pairs with what each is for.  layout "both" or "hashed" (a map
the dense layout refuses).

MEASURED_F64_ERROR: the worst relative error of the f64 loop form (ndt_reference.weights) against ndt_reference.weights_exact per
family, measured by test_ndt_reference_cpu.py (which fails if a figure here is smaller than what it measures, or more than four times
larger) and rounded UP to two digits (cell_counts measures 5.502e-16).  test_gpu_ndt_edges.py derives the device's tolerance from it.
Six of the seven figures are a few 2^-53: at |u| = 2^31 (hashed_ends) an ulp of u is 5e-7 m, but u itself - and with it the error
e = u - mean - is an INPUT of the exact form, rounded as the reference rounds it, so that cancellation is in neither side's error.
conditioning is the exception: the inverse amplifies the rounding of S by cond(S), 1e12 at the last step - 7e-6.
"""
import functools
import math
from fractions import Fraction

import numpy as np

import ndt_reference as ref

MEASURED_F64_ERROR = {
    "axis_edges": 3.2e-16,
    "rotated_edges": 4.4e-16,
    "box_edges": 3.1e-16,
    "far_poses": 2.0e-16,
    "hashed_ends": 2.2e-16,
    "cell_counts": 5.6e-16,
    "conditioning": 7.0e-06,
}

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
REACH_3 = ((0, 0), (2, 0), (-2, 0), (0, 3), (-1, -3))  # test_gpu_ndt.py's
REACH_2 = ((-2, 0), (2, 0), (0, -2), (0, 2), (0, 0))
ONE_SIDED = ((3, 0),)
FAR_OFFSETS = ((0, 0), (64, 0), (-64, 0))
QUARTER_TURNS = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))


class Case:
    def __init__(self, tag, keys, resolution, states, cell_means, cell_covs, pairs, kernel=ref.DEFAULT_KERNEL, minimum=0.01, d1=1.0, d2=0.6,
                 layout="both", spread=1.5, map_cells=None, seed=0, map_seed=0):
        self.tag, self.resolution, self.kernel, self.layout = tag, float(resolution), tuple(kernel), layout
        self.minimum, self.d1, self.d2 = minimum, d1, d2
        self.keys = np.asarray(keys, dtype=np.int64).reshape(-1, 2)
        self.means, self.covs = map_cells if map_cells is not None else ref.revealing_map(self.keys, resolution, spread, map_seed)
        self.states = np.asarray(states, dtype=np.float64).reshape(-1, 4)
        self.cell_means = np.asarray(cell_means, dtype=np.float64).reshape(-1, 2)
        self.cell_covs = np.asarray(cell_covs, dtype=np.float64).reshape(-1, 2, 2)
        self.pairs = pairs
        self.w0 = np.random.Generator(np.random.PCG64(1000 + seed)).uniform(0.5, 1.5, len(self.states))
        self.reach = max(1, max(max(abs(a), abs(b)) for a, b in self.kernel))
        self.wide = map_cells is None and spread >= 2.0**30  # covariances as wide as int32: such a map shows WHETHER a cell was found, not which

    def ref_map(self):
        return ref.NdtMap(self.keys, self.means, self.covs, self.resolution)

    def model(self):
        return dict(minimum_likelihood=self.minimum, d1=self.d1, d2=self.d2, kernel=self.kernel)

    def exact(self, variant=ref.REFERENCE):
        return ref.weights_exact(self.ref_map(), self.states, self.cell_means, self.cell_covs, self.w0, variant=variant, **self.model())

    def loop(self):
        return self.w0 * ref.weights(self.ref_map(), self.states, self.cell_means, self.cell_covs, self.minimum, self.d1, self.d2, self.kernel)


def reveals(case, pairs=None):
    """The smallest relative change of an engineered measurement cell's likelihood when its centre moves one cell - along the engineered
    axis where the pair names one, else along either axis - either way - and finds ANOTHER SET of cells there (f64 loop form; where the
    kernel finds the same cells from both centres, as around a one-cell map, the centre does not enter the likelihood at all).  Pairs
    whose centre finds no cell are left out: there the likelihood is the floor, and what is held is that it stays the floor (the box
    mutants)."""
    m = case.ref_map()
    worst = math.inf
    for p in case.pairs if pairs is None else pairs:
        st, mean, cov = case.states[p["state"]], case.cell_means[p["cell"]], case.cell_covs[p["cell"]]
        tm, tc = ref.transform_cell(st, mean, cov)
        centre = m.cell_near(tm)
        if None in centre:
            continue

        def total(c):
            return sum(ref.cell_likelihood(*m.data[k], tm, tc, case.d1, case.d2) for k in ref.neighbours(m, case.kernel, c) if k)

        here = total(centre)
        if here == 0.0:
            continue
        steps = {"x": ((1, 0), (-1, 0)), "y": ((0, 1), (0, -1)), "xy": ((1, 0), (-1, 0), (0, 1), (0, -1))}[p.get("axis", "xy")]
        found = set(ref.neighbours(m, case.kernel, centre))
        for dx, dy in steps:
            there = (centre[0] + dx, centre[1] + dy)
            if set(ref.neighbours(m, case.kernel, there)) != found:
                worst = min(worst, abs(total(there) - here) / here)
    return worst


def revealing_case(*args, **kw):
    """The Case on the revealing map, of eight by their seeds, on which a centre one cell off moves the engineered likelihoods most."""
    return max((Case(*args, map_seed=map_seed, **kw) for map_seed in range(8)), key=reveals)


def stepped(v, j):
    """The double j ulps above (j > 0) or below v."""
    v = np.float64(v)
    for _ in range(abs(j)):
        v = np.nextafter(v, np.inf if j > 0 else -np.inf)
    return v


def edge(k, resolution, j=0):
    """The double k * resolution (one rounded product), j ulps to a side."""
    return stepped(np.float64(k) * np.float64(resolution), j)


def solve(a, target):
    """x with fl(a + x) == target, next to target - a; None if no neighbouring double does it."""
    a, target = np.float64(a), np.float64(target)
    x = target - a
    for d in (0, 1, -1, 2, -2, 3, -3, 4, -4):
        if a + stepped(x, d) == target:
            return float(stepped(x, d))
    return None


def edge_target(k, resolution, j, a):
    """edge(k, resolution, j); around k = 0 the doubles next to 0 are out of reach of a sum with `a`, so there the nearest values
    a + x can take: one ulp of a to the side of j."""
    return edge(k, resolution, j) if k != 0 or j == 0 else np.float64(a) + stepped(-np.float64(a), j)


def cell_covariances(count, resolution, seed, size=0.4):
    """Well-conditioned measurement covariances, about (size resolution)^2."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.empty((count, 2, 2))
    for i in range(count):
        l1, l2 = rng.uniform(0.5, 2.0, 2) * (size * resolution) ** 2
        a = rng.uniform(0.0, math.pi)
        b = (l1 - l2) * math.cos(a) * math.sin(a)
        out[i] = [[l1 * math.cos(a) ** 2 + l2 * math.sin(a) ** 2, b], [b, l1 * math.sin(a) ** 2 + l2 * math.cos(a) ** 2]]
    return out


def keys_around(centres, half=2, holes=True):
    """Every key within `half` cells of a centre, but for a few holes (never a centre itself)."""
    centres = {(int(x), int(y)) for x, y in centres}
    out = set()
    for cx, cy in centres:
        for dx in range(-half, half + 1):
            for dy in range(-half, half + 1):
                k = (cx + dx, cy + dy)
                if k in centres or not holes or (3 * k[0] + 5 * k[1]) % 11 != 4:
                    out.add(k)
    return np.array(sorted(out), dtype=np.int64)


def rotated(c, s, m):
    """(c mx - s my, s mx + c my), each product and the difference (sum) rounded: the pose's rotation of a cell mean before + t."""
    c, s, mx, my = np.float64(c), np.float64(s), np.float64(m[0]), np.float64(m[1])
    return c * mx - s * my, s * mx + c * my


# ---- axis_edges --------------------------------------------------------------------------------------------------------------------------
AXIS_RESOLUTIONS = (1.0, 0.5, 0.1, 0.05, 0.3, 0.7)


def floors_of(u, resolution):
    """floor(u * inv), floor(u / resolution) in f64, and the floor of the real quotient u / resolution."""
    u, r = np.float64(u), np.float64(resolution)
    return (int(np.floor(u * (np.float64(1.0) / r))), int(np.floor(u / r)), math.floor(Fraction(float(u)) / Fraction(float(r))))


def special_edges(resolution, span=12, most=4):
    """(k, j) with |k| <= span, j in -1 .. 1, where the floors differ: first those where u * inv and u / res do, then those where the
    rounded product and the real quotient do."""
    divide, real = [], []
    for k in sorted(range(-span, span + 1), key=abs):
        for j in (0, -1, 1):
            a, b, c = floors_of(edge(k, resolution, j), resolution)
            if a != b and len(divide) < most:
                divide.append((k, j))
            elif a != c and len(real) < most:
                real.append((k, j))
    return divide, real


@functools.lru_cache(maxsize=None)
def axis_edges():
    cases = []
    for number, resolution in enumerate(AXIS_RESOLUTIONS):
        divide, real = special_edges(resolution)
        targets = divide + real + [(k, j) for k in (-3, 0, 2) for j in (-1, 0, 1)]
        K = 6
        rng = np.random.Generator(np.random.PCG64(50 + number))
        cell_means = np.round(rng.uniform(-1.5, 1.5, (K, 2)) * 64) / 64 * 2.0 ** math.floor(math.log2(resolution))  # few bits, of the cells' size
        states, pairs = [], []
        for t, (k, j) in enumerate(targets):
            for axis in ("x", "y", "xy"):
                i = len(states)
                other = (int(rng.integers(-4, 5)) + 0.375) * resolution
                for turn in range(4 * K):  # the first quarter turn and cell, from this state's own on, whose sums reach the targets
                    c, s = QUARTER_TURNS[(i + turn) % 4]
                    cell = (i + turn // 4) % K
                    ax, ay = rotated(c, s, cell_means[cell])
                    tx = edge_target(k, resolution, j, ax) if "x" in axis else np.float64(other)
                    ty = edge_target(k, resolution, j, ay) if "y" in axis else np.float64(other)
                    x, y = solve(ax, tx), solve(ay, ty)
                    if x is not None and y is not None:
                        break
                assert x is not None and y is not None, (resolution, k, j, axis)
                states.append((c, s, x, y))
                pairs.append(dict(state=i, cell=cell, axis=axis, k=k, ulp=j, target=(tx, ty), divide=(k, j) in divide, real=(k, j) in real))
        assert len(states) <= 64
        centres = [ref.centre_key(ref.NdtMap(np.zeros((0, 2)), [], [], resolution), states[p["state"]], cell_means[p["cell"]])[2] for p in pairs]
        cases.append(revealing_case("axis_edges[%g]" % resolution, keys_around(centres), resolution, states, cell_means,
                          cell_covariances(K, resolution, 60 + number), pairs, seed=number))
    return cases


# ---- rotated_edges -----------------------------------------------------------------------------------------------------------------------
ROTATED_RESOLUTIONS = (1.0, 0.5, 0.1, 0.3)
FLIPS_PER_VARIANT = 10  # per case: 40 of each fused variant over the family


@functools.lru_cache(maxsize=None)
def rotated_edges():
    """General (c, s); the pose's x (y) solved so that the rounded ux (uy) sits on a cell edge or one ulp below it, and kept only where ONE
    fused product in that component lands in another cell than the separately rounded ones.  |mean| is of the size of |u|: an ulp of
    the rotated mean is then an ulp or two of u."""
    cases = []
    for number, resolution in enumerate(ROTATED_RESOLUTIONS):
        rng = np.random.Generator(np.random.PCG64(70 + number))
        K = 8
        scale = 6.0 * resolution
        cell_means = rng.uniform(0.5, 1.0, (K, 2)) * rng.choice([-1.0, 1.0], (K, 2)) * scale
        states, pairs = [], []
        empty = ref.NdtMap(np.zeros((0, 2)), [], [], resolution)
        for name in ref.FUSED_MUTANTS:
            found = 0
            while found < FLIPS_PER_VARIANT:
                theta = rng.uniform(-math.pi, math.pi)
                c, s = np.float64(math.cos(theta)), np.float64(math.sin(theta))
                cell = int(rng.integers(K))
                k, j = int(rng.integers(-6, 7)), int(rng.integers(-1, 1))
                ax, ay = rotated(c, s, cell_means[cell])
                other = np.float64((int(rng.integers(-6, 7)) + 0.375) * resolution)
                on_x = name.startswith("fused_ux")
                x = solve(ax, edge(k, resolution, j) if on_x else other)
                y = solve(ay, other if on_x else edge(k, resolution, j))
                if x is None or y is None:
                    continue
                state = (c, s, x, y)
                plain = ref.centre_key(empty, state, cell_means[cell])[2]
                fused = ref.centre_key(empty, state, cell_means[cell], ref.MUTANTS[name])[2]
                if plain == fused:
                    continue
                pairs.append(dict(state=len(states), cell=cell, axis="x" if on_x else "y", k=k, ulp=j, flips=name, plain=plain, fused=fused,
                                  target=(edge(k, resolution, j) if on_x else other, other if on_x else edge(k, resolution, j))))
                states.append(state)
                found += 1
        centres = [p["plain"] for p in pairs] + [p["fused"] for p in pairs]
        cases.append(revealing_case("rotated_edges[%g]" % resolution, keys_around(centres), resolution, states, cell_means,
                          cell_covariances(K, resolution, 80 + number), pairs, seed=10 + number))
    return cases


# ---- box_edges ---------------------------------------------------------------------------------------------------------------------------
def _box_case(tag, keys, kernel, resolution, seed, spread=1.5):
    """Centre keys reach - 1, reach and reach + 1 cells outside the keys' box: the middle of each side and the four corners."""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 2)
    reach = max(1, max(max(abs(a), abs(b)) for a, b in kernel))
    x0, y0, x1, y1 = keys[:, 0].min(), keys[:, 1].min(), keys[:, 0].max(), keys[:, 1].max()
    xm, ym = (x0 + x1) // 2, (y0 + y1) // 2
    K = 3
    rng = np.random.Generator(np.random.PCG64(seed))
    cell_means = rng.uniform(-2.0, 2.0, (K, 2)) * resolution
    states, pairs = [], []
    for out in (reach - 1, reach, reach + 1):
        places = {"x_lo": (x0 - out, ym), "x_hi": (x1 + out, ym), "y_lo": (xm, y0 - out), "y_hi": (xm, y1 + out),
                  "lo_lo": (x0 - out, y0 - out), "hi_lo": (x1 + out, y0 - out), "lo_hi": (x0 - out, y1 + out), "hi_hi": (x1 + out, y1 + out)}
        for where, (cx, cy) in places.items():
            i = len(states)
            theta = rng.uniform(-math.pi, math.pi)
            c, s = np.float64(math.cos(theta)), np.float64(math.sin(theta))
            cell = i % K
            ax, ay = rotated(c, s, cell_means[cell])
            states.append((c, s, float(np.float64((cx + 0.4375) * resolution) - ax), float(np.float64((cy + 0.5625) * resolution) - ay)))
            pairs.append(dict(state=i, cell=cell, where=where, outside=int(out), reach=int(reach), centre=(int(cx), int(cy))))
    return Case(tag, keys, resolution, states, cell_means, cell_covariances(K, resolution, seed + 1), pairs, kernel=kernel, spread=spread,
                seed=seed)


@functools.lru_cache(maxsize=None)
def box_edges():
    block = [(x, y) for x in range(2, 7) for y in range(-3, 2)]
    cases = [_box_case("box_edges[%s]" % name, block, kernel, 0.5, 90 + n)
             for n, (name, kernel) in enumerate([("default", ref.DEFAULT_KERNEL), ("single", ((0, 0),)), ("reach3", REACH_3),
                                                 ("reach2", REACH_2), ("one_sided", ONE_SIDED)])]
    cases.append(_box_case("box_edges[far_offsets]", [(0, 0), (64, 0)], FAR_OFFSETS, 1.0, 100, spread=40.0))
    cases.append(_box_case("box_edges[one_cell]", [(4, -2)], ref.DEFAULT_KERNEL, 0.3, 102))
    cases.append(_box_case("box_edges[one_row]", [(x, 3) for x in range(6)], REACH_2, 0.7, 104))
    return cases


# ---- far_poses ---------------------------------------------------------------------------------------------------------------------------
FAR_INT32 = (1e4, 1e5, 1e6, 1e7, 1e8, 1e9)                 # keys still int32 at resolution 1
FAR_BEYOND = (2.0**32, 2.0**33, 1e10, 1e15, 1e100, 1e300)   # the reference's cast is undefined; the device's contract: the minimum
NOT_FINITE = (math.inf, math.nan)                           # poses that are not finite: the same contract


@functools.lru_cache(maxsize=None)
def far_poses():
    keys = [(x, y) for x in range(-2, 4) for y in range(-2, 3)]
    K = 4
    cell_means = np.array([(0.4375, 0.5625), (1.25, -0.75), (-0.5, 0.375), (2.5, 1.5)])
    cases = []
    for tag, distances in (("int32", FAR_INT32), ("beyond", FAR_BEYOND), ("not_finite", NOT_FINITE)):
        rng = np.random.Generator(np.random.PCG64(110))
        states, pairs = [(1.0, 0.0, 0.0, 0.0)], []  # (one pose on the map: the family's weights are not the floor's alone)
        for d in distances:
            for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)):
                theta = rng.uniform(-math.pi, math.pi) if len(states) % 2 else 0.0
                # (2^32 and 2^33 with a pose that would be ON the map if a key wrapped to int32; 0 * inf is NaN, so a pose at infinity
                # along one axis is written as such, not multiplied out)
                x, y = (sx * d + 0.5 if sx else 0.5), (sy * d + 0.25 if sy else 0.25)
                states.append((math.cos(theta), math.sin(theta), x, y))
                pairs.extend(dict(state=len(states) - 1, cell=j, distance=d) for j in range(K))
        # beyond int32 on a map whose cells reach as far as the poses lie (covariances of 2^31 cells): a cell found through a wrapped key
        # would COUNT there - on an ordinary map it lies 2^32 m away and adds nothing
        cases.append(Case("far_poses[%s]" % tag, keys, 1.0, states, cell_means, cell_covariances(K, 1.0, 111), pairs, seed=20,
                          spread=2.0**31 if tag == "beyond" else 1.5))
    return cases


# ---- hashed_ends -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hashed_ends():
    """Keys at the ends of int32 at resolution 1 (u * inv is exact): centres on every stored key, one cell beyond int32 (the centre box has
    a border of reach there too) and neighbours that step over either end.  Hashed layout only."""
    lo, hi = INT32_MIN, INT32_MAX
    keys = [(lo, lo), (lo + 1, lo), (lo, lo + 1), (hi, hi), (hi - 1, hi), (hi, hi - 1), (lo, hi), (hi, lo), (lo + 1, hi - 1), (hi - 1, lo + 1)]
    K = 3
    cell_means = np.array([(0.25, 0.5), (-0.75, 0.125), (0.5, -0.375)])
    cases = []
    # "wide": covariances of 2^31 cells, so that a cell at the OTHER end of int32 - which a wrapped neighbour key finds - adds a visible term
    for tag, kernel, spread in (("default", ref.DEFAULT_KERNEL, 1.5), ("reach2", ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (2, 2), (-2, -2)), 1.5),
                                ("wide", ref.DEFAULT_KERNEL, 2.0**31)):
        states, pairs = [], []
        centres = list(keys) + [(lo - 1, lo), (hi + 1, hi), (lo, lo - 1), (hi, hi + 1), (lo - 1, hi + 1), (hi + 1, lo - 1)]
        for cx, cy in centres:
            i = len(states)
            c, s = QUARTER_TURNS[i % 4]
            cell = i % K
            ax, ay = rotated(c, s, cell_means[cell])
            x, y = float(np.float64(cx + 0.5) - ax), float(np.float64(cy + 0.5) - ay)
            states.append((c, s, x, y))
            pairs.append(dict(state=i, cell=cell, centre=(cx, cy)))
        cases.append((Case if spread > 2 else revealing_case)("hashed_ends[%s]" % tag, keys, 1.0, states, cell_means, cell_covariances(K, 1.0, 121), pairs, kernel=kernel,
                          layout="hashed", seed=30, spread=spread))
    return cases


# ---- cell_counts -------------------------------------------------------------------------------------------------------------------------
CELL_COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 129)
SPAN_LOG = 13.0 * math.log(10.0)  # the terms of one pose: from about 1 down to 10^-13


@functools.lru_cache(maxsize=None)
def cell_counts():
    """One map cell, a single-offset kernel, no floor: measurement cell j of K lies so far from the map cell's mean that its term is about
    10^(-13 j / (K - 1)), in shuffled order - the order of the sum shows in the last bits.  K over the wave kernel's blocks of four, its
    64-cell pass and its tail."""
    map_mean, map_var, cell_var, d2 = np.array([[0.5, 0.5]]), 0.05**2, 0.03**2, 1.0
    cases = []
    for K in CELL_COUNTS:
        rng = np.random.Generator(np.random.PCG64(130 + K))
        share = rng.permutation(K) / max(K - 1, 1)
        distance = np.sqrt(2.0 * SPAN_LOG * share * (map_var + cell_var) / d2)  # at most 0.44: inside the cell
        angle = rng.uniform(0.0, 2 * math.pi, K)
        cell_means = map_mean + np.stack([distance * np.cos(angle), distance * np.sin(angle)], 1)
        cell_covs = np.tile(np.eye(2) * cell_var, (K, 1, 1))
        states = [(math.cos(t), math.sin(t), 0.5 - (0.5 * math.cos(t) - 0.5 * math.sin(t)) + dx, 0.5 - (0.5 * math.sin(t) + 0.5 * math.cos(t)) + dy)
                  for t, dx, dy in ((0.0, 0.0, 0.0), (0.01, 0.003, -0.002), (-0.02, -0.004, 0.001), (0.015, 0.0, 0.004), (-0.005, 0.002, 0.002))]
        cases.append(Case("cell_counts[%d]" % K, [(0, 0)], 1.0, states, cell_means, cell_covs, [dict(cells=K)], kernel=((0, 0),), minimum=0.0,
                          d1=1.0, d2=d2, map_cells=(map_mean, np.eye(2)[None] * map_var), seed=40 + K))
    return cases


# ---- conditioning and singular ----------------------------------------------------------------------------------------------------------------
def along_diagonal(wide, thin):
    """The covariance with variance `wide` along (1, 1) and `thin` across it."""
    return np.array([[(wide + thin) / 2, (wide - thin) / 2], [(wide - thin) / 2, (wide + thin) / 2]])


CONDITIONS = tuple(10.0**d for d in range(13))


@functools.lru_cache(maxsize=None)
def conditioning():
    """cond(S' + S_map) from 1 to 1e12: the measurement's and the map cell's covariances thin along the same diagonal (half of the sum
    each), the error 0, 1, 2 and 3 standard deviations across the thin direction.  Rotations by 0 and pi only: R S R^T = S exactly."""
    cases = []
    wide = 0.02
    for cond in CONDITIONS:
        thin = wide / cond
        map_mean = np.array([[0.5, 0.5]])
        sigma = math.sqrt(thin)
        offsets = np.array([t * sigma * np.array([1.0, -1.0]) / math.sqrt(2.0) for t in (0.0, 1.0, 2.0, 3.0)])
        cell_means = map_mean + offsets
        cell_covs = np.tile(along_diagonal(wide / 2, thin / 2), (4, 1, 1))
        states = [(1.0, 0.0, 0.0, 0.0), (1.0, 0.0, 0.25 * sigma, -0.25 * sigma), (-1.0, 0.0, 1.0, 1.0), (1.0, 0.0, 0.001, 0.001)]
        cases.append(Case("conditioning[%g]" % cond, [(0, 0)], 1.0, states, cell_means, cell_covs, [dict(cond=cond)], kernel=((0, 0),),
                          minimum=0.0, d1=1.0, d2=1.0, map_cells=(map_mean, along_diagonal(wide / 2, thin / 2)[None]), seed=60))
    return cases


def collinear_covariance(ts):
    """ndt_reference.fit_points of points (t, t) on a 45-degree line, without the clamp's effect (variance well above 1e-5): all four
    entries are the same double, the determinant is exactly 0."""
    return ref.fit_points(np.stack([ts, ts], 1))[1]


SINGULAR_ROTATIONS = 12


@functools.lru_cache(maxsize=None)
def singular():
    """Covariances of exactly collinear points in the map (a 45-degree wall) and in the measurement.  Cells 0 .. 3 lie on a 45-degree line
    in the base frame too: under the identity and a half turn S' + S_map has four equal entries and det == 0 exactly - with e == 0, e
    along the wall, e across it and a general e.  Cell 4 + r is a wall seen under rotation r: its points lie on the line that pose 2 + r
    turns onto 45 degrees, so det(S' + S_map) is rounding noise of either sign there, and e lies across the wall.  What the f64
    arithmetic of ndt_cell_likelihood gives for each (state, cell) - NaN (0 * inf, inf - inf), +inf (a tiny negative det under a
    positive form), 0 or a finite term - is read off by the loop form, which runs the kernel's operations in the kernel's order
    (singular_terms)."""
    ts = np.array([0.0, 0.125, 0.25, 0.5, 0.625, 1.0])
    S = collinear_covariance(ts)
    assert S[0, 0] == S[0, 1] == S[1, 0] == S[1, 1]
    map_mean = np.array([0.5, 0.5])
    cell_means = [(0.5, 0.5), (0.625, 0.625), (0.5625, 0.4375), (0.75, 0.5)]  # e == 0; e along the line; e across it; e general
    cell_covs = [collinear_covariance(ts * 0.5)] * 4
    states = [(1.0, 0.0, 0.0, 0.0), (-1.0, 0.0, 1.0, 1.0)]
    rng = np.random.Generator(np.random.PCG64(140))
    wanted = {-1: SINGULAR_ROTATIONS // 3, 0: SINGULAR_ROTATIONS // 3, 1: SINGULAR_ROTATIONS // 3}  # by the sign of the f64 det
    while any(wanted.values()):
        t = rng.uniform(-math.pi, math.pi)
        c, s = math.cos(t), math.sin(t)
        along = np.array([math.cos(math.pi / 4 - t), math.sin(math.pi / 4 - t)])  # R(t) along = (1, 1) / sqrt 2
        cov = ref.fit_points(np.outer(ts * 0.5, along))[1]
        total = ref.transform_cell((c, s, 0.0, 0.0), (0.0, 0.0), cov)[1] + S
        sign = int(np.sign(total[0, 0] * total[1, 1] - total[1, 0] * total[0, 1]))
        if not wanted[sign]:
            continue
        wanted[sign] -= 1
        r = len(states)
        mean = rng.uniform(-0.5, 0.5, 2)
        across = np.array([1.0, -1.0]) * 0.0625 * (1 + r % 3)
        cell_covs.append(cov)
        cell_means.append(mean)
        states.append((c, s, map_mean[0] + across[0] - (c * mean[0] - s * mean[1]), map_mean[1] + across[1] - (s * mean[0] + c * mean[1])))
    return [Case("singular", [(0, 0)], 1.0, states, cell_means, cell_covs, [], kernel=((0, 0),), minimum=0.01, d1=1.0, d2=1.0,
                 map_cells=(map_mean[None], S[None]), seed=70)]


def singular_terms(case):
    """Per (state, cell): the f64 term of the loop form before the max - NaN, +inf or finite - and det's sign."""
    m = case.ref_map()
    out = np.empty((len(case.states), len(case.cell_means)))
    for i, st in enumerate(case.states):
        for j, (mean, cov) in enumerate(zip(case.cell_means, case.cell_covs)):
            tm, tc = ref.transform_cell(st, mean, cov)
            out[i, j] = ref.likelihood_at(m, tm, tc, -math.inf, case.d1, case.d2, case.kernel)
    return out


def device_rule(case):
    """The device's weights on `singular` by its written rule: a NaN term counts as the minimum (the kernel's select), an
    infinite term makes the weight infinite."""
    terms = singular_terms(case)
    held = np.where(np.isnan(terms), case.minimum, np.maximum(np.nan_to_num(terms, nan=0.0, posinf=np.inf), case.minimum))
    return case.w0 * (1.0 + held.sum(axis=1))


FAMILIES = {"axis_edges": axis_edges, "rotated_edges": rotated_edges, "box_edges": box_edges, "far_poses": far_poses,
            "hashed_ends": hashed_ends, "cell_counts": cell_counts, "conditioning": conditioning, "singular": singular}
EXACT_FAMILIES = tuple(name for name in FAMILIES if name != "singular")
WELL_CONDITIONED = ("axis_edges", "rotated_edges", "box_edges", "far_poses", "hashed_ends")
