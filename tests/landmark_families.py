"""Engineered cases for the landmark and bearing reweight kernels (beluga_amd/csrc/landmark_kernels.hip), the inputs of
tests/test_landmark_reference_cpu.py and tests/test_gpu_landmark_edges.py.  A case is a map, at most 64 states with prior weights that are
not 1, detections and parameters.  FAMILIES are held to landmark_reference.weights_exact, RULE_FAMILIES to the f64 sequence itself.

near_ties (landmark model)  a pair A, B of one category around the detection's world point p (the f64 point the kernels form) whose f64
    squared distances are `equal` to the bit while the exact ones differ, one `ulp` apart in the order of the exact ones, or `inverted`:
    ordered one way in f64 and the other way exactly.  A lies along the detection's bearing, B off it, so the pick moves the term by far
    more than 1e-3 of it.  The pair stands at the map-order placements (0, 1), (0, g), (g - 1, g), (5, 129), (64, 65) of a category of
    130 whose other members are far away, in both orders, for k in 1, 2, 8, 33 (g = 64, 32, 8, 1; the k detections are the same one), and
    the cases cycle through identity / axis-aligned / general rotation, near the origin / at UTM scale, and the three kinds, so every
    combination of those three stands at one k x placement, once with A first and once with B first.  Near the origin B is nudged by ulps; at UTM scale one ulp of a coordinate
    moves d2 by about 1e6 of its ulps, so there A and B sit on the lattice p + 2^-30 Z^3, where l - p is exact, and the lattice is
    searched for near-equal squared norms.
range_leaks (both models)  categories 0, 1, 7, 8, 9, 0xFFFFFFFE, 0xFFFFFFFF of 1, 2, 63, 64, 65, 130 and 1 landmarks, interleaved in map
    order.  For the first state the LAST landmark (in map order) of the category below a detected one and the FIRST of the category
    above it sit exactly on the detection's world point (exactly along its bearing in the bearing model): a scan one landmark early or
    late finds a perfect match, while the category's own best is clearly worse.  Categories 5 and 10 have no landmark and sit between two
    that have.  k covers 1, 3, 4, 5, 33, 64; the bearing cases have several detections per category with the categories descending in
    the caller's order, one case with all 64 detections of one category, and one with a category the map does not have (every weight 0).
degenerate_vectors  a zero detection, a landmark exactly at the robot / at the (tilted) sensor's origin, apertures of exactly 0 and
    exactly pi, a vertical bearing.  All exact: normalized() of an exactly zero vector is the vector and atan2(0, 0) = 0.
tiny_weights  small sigmas and up to 64 detections: exact weights in [1e-290, 1e-200], in the denormal range and below it; terms that
    underflow to exactly 0 with random_prob = 0, and random_prob = 1e-3 beside them.  The comparison gains an absolute part of (k + 2)
    denormal steps; an exact weight below 2^-1075 must come out as +0; no NaN, no negative zero.
far_maps  UTM-scale maps (5e5 m, 4e6 m), 16 detections, ordinary sigmas: the largest cost of f64, through range_error's cancellation.

RULE_FAMILIES - where the f64 sequence and the real value part ways, the sequence IS the contract, read off
landmark_match_term, bearing_of and normalized() in landmark_kernels.hip, which is also what Eigen's normalized() does in the reference:
overflow_underflow  a detection of length 1e150: its squared norm is +inf, so range = +inf and unit = d / inf is a vector of signed
    zeros; the aperture is atan2(0, +-0) = 0 or pi by the sign of the zero dot product, the landmark term exp(-inf) * exp(..) + random_prob
    = random_prob, the bearing term 1 or exp(-pi^2 / den).  A detection of length 1e-160: the
    squared norm underflows to 0, so range = 0 and unit = d itself; |unit x b|^2 underflows to 0 as well and the aperture is atan2(0, +-tiny)
    = 0 or pi by the sign of the dot product.
not_finite_poses  poses at +-inf, NaN and 1e300.  A pose with an inf or a NaN gives a NaN weight in either model (inf - inf, inf / inf or
    0 * inf on the way to the term) unless no detection's category has a landmark; at 1e300 every squared distance is +inf, the first
    landmark of the category is kept, the robot-frame landmark normalises to signed zeros: the landmark term is random_prob, the bearing
    term 1 or exp(-pi^2 / den) (atan2(0, +0) = 0, atan2(0, -0) = pi).
    Lane and wave forms agree in class: with NaN candidates the wave reduction may keep another index than the lane scan's first (NaN is
    outside pick_beats' total order), but the term is NaN for ANY landmark then, and an index is only ever taken from a lane that
    scanned (at < count), never formed from a value.
"""
import dataclasses
import functools
import math
from fractions import Fraction

import numpy as np

import landmark_reference as ref

# The worst relative error of the f64 loop form (libm) against weights_exact per family, beyond the family's absolute part; measured by
# tests/test_landmark_reference_cpu.py, which refuses a figure here that is below what it measures.
MEASURED_F64_ERROR = {
    "near_ties": 4e-14,
    "range_leaks": 2.3e-14,
    "degenerate_vectors": 2.5e-15,
    "tiny_weights": 9e-12,
    "far_maps": 5.8e-10,
}


@dataclasses.dataclass
class Case:
    tag: str
    bearing: bool
    positions: np.ndarray
    categories: np.ndarray
    states: np.ndarray
    w0: np.ndarray
    det: np.ndarray
    dcat: np.ndarray
    params: dict
    meta: dict = dataclasses.field(default_factory=dict)

    @property
    def k(self):
        return len(self.det)

    def ref_map(self):
        return ref.LandmarkMap(self.positions, self.categories)

    def loop(self, variant=ref.PLAIN, wave=False):
        return ref.weights_loop(self.ref_map(), self.states, self.det, self.dcat, self.w0, self.bearing, variant=variant, wave=wave, **self.params)

    def exact(self):
        return ref.weights_exact(self.ref_map(), self.states, self.det, self.dcat, self.w0, self.bearing, **self.params)

    def absolute_steps(self):
        return self.k + 2 if self.meta.get("tiny") else 0


def _w0(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).uniform(0.5, 2.0, n)


def _u32(values):
    return np.asarray(values, dtype=np.uint32)


def pose(theta, x, y):
    return (math.cos(theta), math.sin(theta), x, y)


# ---- near_ties ---------------------------------------------------------------------------------------------------------------------------
TIE_KS = (1, 2, 8, 33)
TIE_POSES = {"identity": (1.0, 0.0), "axis": (0.0, 1.0), "general": (math.cos(0.7), math.sin(0.7))}
TIE_OFFSETS = {"origin": (0.5, -0.25), "utm": (500123.25, 4000321.5)}
TIE_KINDS = ("equal", "ulp", "inverted")
TIE_DETECTION = (3.0, 1.0, 0.25)
TIE_RADIUS = 2.0
TIE_PARAMS = dict(sigma_range=2.0, sigma_bearing=0.25, random_prob=1e-4)
LATTICE = 2.0**-30


def d2_f64(l, p):
    return ref.squared_distance(tuple(float(v) for v in l), tuple(float(v) for v in p))


def d2_exact(l, p):
    return sum((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(l, p))


def tie_kind(a, b, p):
    """The kind of the pair (a, b) about p, or None."""
    fa, fb, ea, eb = d2_f64(a, p), d2_f64(b, p), d2_exact(a, p), d2_exact(b, p)
    if ea == eb:
        return None
    if fa == fb:
        return "equal"
    if (fa < fb) != (ea < eb):
        return "inverted"
    return "ulp" if abs(fa - fb) == np.spacing(min(fa, fb)) else None


def _frame(state, p):
    """Unit vectors at p: along the bearing from the robot, and horizontal across it."""
    v = np.array([p[0] - state[2], p[1] - state[3], p[2]])
    u = v / np.linalg.norm(v)
    w = np.array([-u[1], u[0], 0.0])
    return u, w / np.linalg.norm(w)


def _nudged_pairs(state, p):
    """Near the origin: A = p + r u, B = p + r w with B's x and y nudged by ulps.  {kind: (A, B)}, the first of each kind in scan order."""
    u, w = _frame(state, p)
    a = np.asarray(p) + TIE_RADIUS * u
    b0 = np.asarray(p) + TIE_RADIUS * w
    fa = d2_f64(a, p)
    span = np.arange(-90, 91)
    I, J = np.meshgrid(span, span, indexing="ij")
    bx, by = b0[0] + I * np.spacing(b0[0]), b0[1] + J * np.spacing(b0[1])
    ex, ey, ez = bx - p[0], by - p[1], b0[2] - p[2]
    fb = ex * ex + (ey * ey + ez * ez)
    near = np.argwhere(np.abs(fb - fa) <= np.spacing(fa))
    found = {}
    for i, j in near:
        b = (float(bx[i, j]), float(by[i, j]), float(b0[2]))
        kind = tie_kind(a, b, p)
        if kind and kind not in found:
            found[kind] = (tuple(float(v) for v in a), b)
            if len(found) == 3:
                break
    return found


def _lattice_pairs(state, p):
    """At UTM scale: A = p + h a, B = p + h b with integer a, b; b1 is scanned, b2 closes the circle from below and b3 = round(sqrt(rest))
    takes what is left, and the candidates whose squared norms differ by at most 4096 (4 ulps of d2 in units of h^2) are classified."""
    u, w = _frame(state, p)
    h = LATTICE
    a = [int(round(TIE_RADIUS * c / h)) for c in u]
    T = a[0] * a[0] + a[1] * a[1] + a[2] * a[2]
    A = tuple(float(p[c] + a[c] * h) for c in range(3))
    assert all(Fraction(A[c]) == Fraction(float(p[c])) + a[c] * Fraction(h) for c in range(3)), "A is off the lattice"
    major, minor = (0, 1) if abs(w[1]) >= abs(w[0]) else (1, 0)  # scan the smaller component of w, solve the larger one
    start = int(round(TIE_RADIUS * w[major] / h))
    found = {}
    for chunk in range(40):
        b1 = start + np.arange(chunk * 20000, (chunk + 1) * 20000, dtype=np.int64)
        rest = T - b1 * b1
        b2 = np.floor(np.sqrt(rest.astype(np.float64))).astype(np.int64)
        b2 -= (b2 * b2 > rest)
        b2 += ((b2 + 1) * (b2 + 1) <= rest)
        R = rest - b2 * b2
        b3 = np.rint(np.sqrt(R.astype(np.float64))).astype(np.int64)
        delta = b3 * b3 - R
        for t in np.flatnonzero((np.abs(delta) <= 4096) & (delta != 0))[:4000]:
            b = [0, 0, int(b3[t])]
            b[major], b[minor] = int(b1[t]), int(b2[t]) * (1 if w[minor] >= 0 else -1)
            B = tuple(float(p[c] + b[c] * h) for c in range(3))
            if any(Fraction(B[c]) != Fraction(float(p[c])) + b[c] * Fraction(h) for c in range(3)):
                continue
            kind = tie_kind(A, B, p)
            if kind and kind not in found:
                found[kind] = (A, B)
        if len(found) == 3:
            break
    return found


@functools.lru_cache(maxsize=None)
def tie_pairs(pose_name, offset_name):
    c, s = TIE_POSES[pose_name]
    state = (c, s) + TIE_OFFSETS[offset_name]
    p = ref.world_point(state, TIE_DETECTION)
    found = _nudged_pairs(state, p) if offset_name == "origin" else _lattice_pairs(state, p)
    assert set(found) == set(TIE_KINDS), "threshold not reached: %s %s finds %s" % (pose_name, offset_name, sorted(found))
    return state, p, found


def tie_placements(k):
    g = ref.group_of(k)
    return sorted({pl for pl in [(0, 1), (0, g), (g - 1, g), (5, 129), (64, 65)] if pl[0] < pl[1]})


@functools.lru_cache(maxsize=None)
def near_ties():
    combos = [(po, of, ki) for of in TIE_OFFSETS for po in TIE_POSES for ki in TIE_KINDS]
    cases, number = [], 0
    for k in TIE_KS:
        for at in tie_placements(k):
            for order in (0, 1):
                # 18 k x placement slots and 18 combinations: a slot takes one combination in both orders, A first and B first (where the
                # f64 distances differ, exactly one of the two orders has the match at the later place)
                pose_name, offset_name, kind = combos[(number // 2) % len(combos)]
                state, p, found = tie_pairs(pose_name, offset_name)
                pair = found[kind] if order == 0 else found[kind][::-1]
                positions = np.array([(p[0] + 1000.0 + i, p[1] + 1000.0, 0.0) for i in range(130)])
                positions[at[0]], positions[at[1]] = pair
                n = 5
                cases.append(Case("near_ties[%s,%s,%s,k=%d,at=%s,order=%d]" % (pose_name, offset_name, kind, k, at, order), False, positions,
                                  _u32([7] * 130), np.tile(state, (n, 1)), _w0(n, number), np.tile(TIE_DETECTION, (k, 1)), _u32([7] * k),
                                  dict(TIE_PARAMS), dict(kind=kind, offset=offset_name, pose=pose_name, at=at, order=order, point=p, along=found[kind][0],
                                                         across=found[kind][1])))
                number += 1
    return cases


# ---- range_leaks -------------------------------------------------------------------------------------------------------------------------
LEAK_SIZES = {0: 1, 1: 2, 7: 63, 8: 64, 9: 65, 0xFFFFFFFE: 130, 0xFFFFFFFF: 1}
LEAK_ABSENT = (5, 10)
LEAK_KS = (1, 3, 4, 5, 33, 64)
LEAK_PARAMS = dict(sigma_range=1.0, sigma_bearing=0.5, random_prob=1e-4)
TILTED = (0.0, math.sin(0.15), 0.0, math.cos(0.15), 0.5, 0.25, 1.0)  # the sensor pitched by 0.3 rad, off the robot's origin
LEAK_BEARING = dict(sigma_bearing=0.5, sensor_pose_in_robot=TILTED)
LEAK_COSINE = 0.95  # a bearing landmark of a detected category points at least acos(0.95) = 0.3176 rad off every bait: a term of exp(-0.2) at the most


def _leak_states(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    first = pose(0.4, 1.0, -2.0)
    others = [pose(rng.uniform(-3.0, 3.0), rng.uniform(-3.0, 3.0), rng.uniform(-3.0, 3.0)) for _ in range(9)]
    order = [first, others[0], first, others[1], others[2], first, others[3], others[4], others[5], first, others[6], others[7], others[8]]
    return np.array(order)


def _leak_vector(cat, bearing):
    """The detection of category `cat` (one per category: a category's bait serves one world point)."""
    present = sorted(LEAK_SIZES) + list(LEAK_ABSENT)
    a = 0.7 * sorted(present).index(cat)
    d = np.array([2.5 * math.cos(a) + 0.25, 2.5 * math.sin(a), 0.5 + 0.125 * (cat % 5)])
    return d / 2.0 if bearing else d


def _bait_point(state, d, bearing, params):
    if not bearing:
        return ref.world_point(tuple(state), tuple(d))
    R, t = ref.sensor_frame(tuple(float(v) for v in state), ref.rotation_matrix(params["sensor_pose_in_robot"][:4]).tolist(),
                            list(params["sensor_pose_in_robot"][4:]))
    # the world point 3 |d| along the bearing: tw + Rw (3 d)
    return tuple(t[r] + 3.0 * (R[3 * r] * d[0] + R[3 * r + 1] * d[1] + R[3 * r + 2] * d[2]) for r in range(3))


def leak_map(bearing, params, seed=3):
    """The map with its baits for the first state: category c's first landmark (map order) sits on the point of the category below,
    its last on the point of the category above."""
    rng = np.random.Generator(np.random.PCG64(seed))
    present = sorted(LEAK_SIZES)
    cat = rng.permutation(np.concatenate([np.full(LEAK_SIZES[c], c, dtype=np.uint32) for c in present])).astype(np.uint32)
    state = _leak_states(seed)[0]
    origin = np.array(_bait_point(state, np.zeros(3), bearing, params))
    # Every landmark is first scattered around the sensor (the robot in the landmark model): within 9 m in x and y, more than 1.5 m from
    # every bait point and, in the bearing map, in a direction from the sensor whose cosine with every bait's direction is below
    # LEAK_COSINE (more than 18 degrees off it).  Then two members of each category are moved onto the neighbours' bait points.
    points = {c: np.array(_bait_point(state, _leak_vector(c, bearing), bearing, params)) for c in present}
    pos = np.zeros((len(cat), 3))
    for i in range(len(cat)):
        while True:
            cand = origin + np.array([rng.uniform(-9.0, 9.0), rng.uniform(-9.0, 9.0), rng.uniform(-1.0, 2.0)])
            far_enough = all(np.linalg.norm(cand - q) > 1.5 for q in points.values())
            off_axis = all(np.dot(cand - origin, q - origin) / (np.linalg.norm(cand - origin) * np.linalg.norm(q - origin)) < LEAK_COSINE for q in points.values())
            if far_enough and (off_axis or not bearing):
                break
        pos[i] = cand
    for n, c in enumerate(present):
        members = np.flatnonzero(cat == c)
        if n > 0:
            pos[members[0]] = points[present[n - 1]]
        if n + 1 < len(present):
            pos[members[-1]] = points[present[n + 1]]
    return pos, cat


@functools.lru_cache(maxsize=None)
def range_leaks():
    cases = []
    states = _leak_states(3)
    choices = sorted(list(LEAK_SIZES) + list(LEAK_ABSENT))
    pos, cat = leak_map(False, LEAK_PARAMS)
    number = 0
    for k in LEAK_KS:
        for start in (range(len(choices)) if k == 1 else (k % len(choices),)):
            dcat = [choices[(start + j) % len(choices)] for j in range(k)]
            det = np.array([_leak_vector(c, False) for c in dcat])
            cases.append(Case("range_leaks[landmark,k=%d,start=%d]" % (k, start), False, pos, cat, states, _w0(len(states), 100 + number), det, _u32(dcat),
                              dict(LEAK_PARAMS), dict(baited=0)))
            number += 1
    pos, cat = leak_map(True, LEAK_BEARING)
    present = sorted(LEAK_SIZES)
    rng = np.random.Generator(np.random.PCG64(17))

    def bearing_case(tag, dcat):
        det, seen = [], set()
        for c in dcat:  # the first detection of a category is the baited one, the others point elsewhere
            if c in seen:
                v = rng.normal(size=3)
                det.append(v / np.linalg.norm(v) * rng.uniform(0.5, 2.0))
            else:
                det.append(_leak_vector(c, True))
                seen.add(c)
        cases.append(Case("range_leaks[bearing,%s]" % tag, True, pos, cat, states, _w0(len(states), 200 + len(cases)), np.array(det), _u32(dcat),
                          dict(LEAK_BEARING), dict(baited=0)))

    for k in LEAK_KS:
        dcat = sorted((present[(k + j) % len(present)] for j in range(k)), reverse=True)  # descending in the caller's order
        bearing_case("k=%d" % k, dcat)
    bearing_case("k=64,one_category", [0xFFFFFFFE] * 64)
    bearing_case("k=5,absent", [9, 8, 5, 1, 0])
    return cases


# ---- degenerate_vectors ------------------------------------------------------------------------------------------------------------------
def _lone_states():
    return np.array([(1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 2.0, -1.0), pose(0.3, 0.5, 0.5), (1.0, 0.0, 2.0, -1.0)])


@functools.lru_cache(maxsize=None)
def degenerate_vectors():
    states = _lone_states()
    # categories: 1 straight ahead of the identity pose, 2 straight behind it, 3 at the robots (0, 0) and (2, -1), 4 overhead, 5 scattered
    pos = np.array([(4.0, 0.0, 0.0), (-4.0, 0.0, 0.0), (0.0, 0.0, 0.0), (2.0, -1.0, 0.0), (0.0, 0.0, 3.0), (1.0, 2.0, 0.5), (-2.0, 1.0, 1.5), (3.0, -3.0, 0.0)])
    cat = _u32([1, 2, 3, 3, 4, 5, 5, 5])
    det = np.array([(2.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 2.0), (1.0, 1.0, 0.0), (0.0, 0.0, 0.0)])
    dcat = _u32([1, 2, 3, 5, 4, 3, 1])
    params = dict(sigma_range=1.5, sigma_bearing=1.25, random_prob=1e-4)
    cases = [Case("degenerate_vectors[landmark]", False, pos, cat, states, _w0(4, 1), det, dcat, params)]
    # level sensor at the robot's origin: apertures of exactly 0 (category 1 ahead) and pi (category 2 behind), vertical bearings, a zero detection
    bdet = np.array([(1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 2.0), (0.5, -0.5, 0.25)])
    bcat = _u32([1, 2, 4, 5, 5, 3])
    cases.append(Case("degenerate_vectors[bearing,level]", True, pos, cat, states, _w0(4, 2), bdet, bcat, dict(sigma_bearing=1.25, sensor_pose_in_robot=ref.IDENTITY_SE3)))
    # tilted sensor: for the two unrotated poses, at (0, 0) and at (2, -1), its origin is robot + (0.5, 0.25, 1.0) exactly.  Category 3 sits on
    # the first pose's sensor origin and category 6 on the second's, each alone in its category: a landmark at the sensor's origin has the
    # zero bearing, whose dot product with any detection is 0, so it is the match only where no other candidate has a positive one.
    tpos = pos.copy()
    tpos[2], tpos[3] = (0.5, 0.25, 1.0), (2.5, -0.75, 1.0)
    tcat = _u32([1, 2, 3, 6, 4, 5, 5, 5])
    cases.append(Case("degenerate_vectors[bearing,tilted]", True, tpos, tcat, states, _w0(4, 3), np.concatenate([bdet, [(1.0, 2.0, -0.5)]]),
                      _u32(list(bcat) + [6]), dict(sigma_bearing=1.25, sensor_pose_in_robot=TILTED)))
    return cases


# ---- tiny_weights ------------------------------------------------------------------------------------------------------------------------
TINY_TRUTH = pose(0.25, 1.0, 2.0)


def _seen_from(state, pos):
    """The landmarks in the robot frame of `state`."""
    c, s, x, y = state
    v = pos - np.array([x, y, 0.0])
    return np.column_stack([c * v[:, 0] + s * v[:, 1], c * v[:, 1] - s * v[:, 0], v[:, 2]])


def _tiny_case(tag, k, sigma_range, sigma_bearing, random_prob, decades, seed, bearing=False, exactly=None):
    """64 states that step away from the truth along x so that log10 of the weight falls about linearly to -decades; exactly: the
    decades of the weight state by state, each met by bisecting the step on the loop form's sum of exponents (random_prob = 0)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pos = np.column_stack([rng.uniform(-6.0, 8.0, 12), rng.uniform(-5.0, 9.0, 12), rng.uniform(0.0, 1.0, 12)])
    cat = _u32(np.arange(12) % 3)
    which = np.arange(k) % 12
    det = _seen_from(TINY_TRUTH, pos)[which]
    sigma = sigma_bearing if bearing else sigma_range
    scale = 0.25 if bearing else 1.0  # (a step of delta metres turns a bearing at about 4 m by about delta / 4)
    delta = np.sqrt(np.linspace(0.0, decades, 64) * math.log(10.0) * 2.0 * sigma * sigma / k) / scale
    at = lambda d: (TINY_TRUTH[0], TINY_TRUTH[1], TINY_TRUTH[2] + d, TINY_TRUTH[3])
    params = dict(sigma_bearing=sigma_bearing, sensor_pose_in_robot=ref.IDENTITY_SE3) if bearing else dict(sigma_range=sigma_range, sigma_bearing=sigma_bearing,
                                                                                                           random_prob=random_prob)
    if exactly is not None:
        lmap, delta = ref.LandmarkMap(pos, cat), []
        for target in exactly:
            lo, hi = 0.0, 1.0
            for _ in range(40):
                mid = 0.5 * (lo + hi)
                total = ref.weights_loop(lmap, [at(mid)], det, cat[which], [1.0], bearing, **params)[2][0]
                lo, hi = (mid, hi) if total < target * math.log(10.0) else (lo, mid)
            delta.append(hi)
    states = np.array([at(d) for d in delta])
    return Case("tiny_weights[%s]" % tag, bearing, pos, cat, states, _w0(len(states), seed), det, _u32(cat[which]), params, dict(tiny=True))


@functools.lru_cache(maxsize=None)
def tiny_weights():
    return [_tiny_case("k=64,decades=450", 64, 0.05, 1.0, 0.0, 450.0, 1),
            _tiny_case("k=64,denormal", 64, 0.05, 1.0, 0.0, 0.0, 2, exactly=np.linspace(300.0, 327.0, 28)),
            _tiny_case("k=33,decades=420", 33, 0.04, 0.5, 0.0, 420.0, 3),
            _tiny_case("k=4,terms_underflow,rp=0", 4, 0.01, 1.0, 0.0, 3000.0, 4),
            _tiny_case("k=4,terms_underflow,rp=1e-3", 4, 0.01, 1.0, 1e-3, 3000.0, 4),
            _tiny_case("k=64,rp=1e-3", 64, 0.01, 1.0, 1e-3, 3000.0, 5),
            _tiny_case("bearing,k=64", 64, 0.0, 0.02, 0.0, 450.0, 6, bearing=True)]


# ---- far_maps ----------------------------------------------------------------------------------------------------------------------------
UTM = (500123.25, 4000321.5)


@functools.lru_cache(maxsize=None)
def far_maps():
    rng = np.random.Generator(np.random.PCG64(9))
    n_l = 96
    pos = np.column_stack([UTM[0] + rng.uniform(-20.0, 20.0, n_l), UTM[1] + rng.uniform(-20.0, 20.0, n_l), rng.uniform(0.0, 2.0, n_l)])
    cat = _u32(rng.integers(0, 6, n_l))
    truth = pose(1.1, UTM[0] + 1.5, UTM[1] - 2.25)
    which = rng.choice(n_l, 16, replace=False)
    seen = _seen_from(truth, pos)[which] + rng.normal(0.0, 0.02, (16, 3))
    states = np.array([pose(1.1 + rng.normal(0.0, 0.05), truth[2] + rng.normal(0.0, 0.2), truth[3] + rng.normal(0.0, 0.2)) for _ in range(32)])
    out = [Case("far_maps[landmark]", False, pos, cat, states, _w0(32, 1), seen, _u32(cat[which]), dict(sigma_range=0.5, sigma_bearing=0.25, random_prob=1e-4))]
    # the level sensor of the bearing model sits 0.5 m up; the bearings are what it sees, unnormalised
    bparams = dict(sigma_bearing=0.1, sensor_pose_in_robot=(0.0, 0.0, 0.0, 1.0, 0.1, 0.0, 0.5))
    bseen = _seen_from(truth, pos)[which] - np.array([0.1, 0.0, 0.5])
    bseen = bseen / np.linalg.norm(bseen, axis=1)[:, None] * rng.uniform(0.5, 2.0, 16)[:, None] + rng.normal(0.0, 0.005, (16, 3))
    out.append(Case("far_maps[bearing]", True, pos, cat, states, _w0(32, 2), bseen, _u32(cat[which]), bparams))
    return out


# ---- the families held to the f64 sequence -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def overflow_underflow():
    states = _lone_states()
    pos = np.array([(4.0, 0.0, 0.0), (-4.0, 1.0, 0.0), (0.5, 3.0, 1.0), (2.0, -2.0, 0.5), (-1.0, -3.0, 1.5)])
    cat = _u32([1, 1, 1, 2, 2])
    det = np.array([(1e150, 0.0, 0.0), (0.0, 1e-160, 0.0), (6e149, -8e149, 1e149), (-1e-160, 1e-161, 0.0), (1.0, 2.0, 0.5), (0.0, 0.0, -1e-160)])
    dcat = _u32([1, 1, 2, 2, 1, 2])
    return [Case("overflow_underflow[landmark]", False, pos, cat, states, _w0(4, 1), det, dcat, dict(sigma_range=1.5, sigma_bearing=1.25, random_prob=1e-3)),
            Case("overflow_underflow[bearing]", True, pos, cat, states, _w0(4, 2), det, dcat, dict(sigma_bearing=1.25, sensor_pose_in_robot=TILTED))]


@functools.lru_cache(maxsize=None)
def not_finite_poses():
    inf, nan = math.inf, math.nan
    c, s = math.cos(0.6), math.sin(0.6)
    states = np.array([pose(0.2, 0.5, -0.5), (1.0, 0.0, inf, 0.0), (1.0, 0.0, 0.0, -inf), (c, s, inf, -inf), (0.0, 1.0, -inf, 1.0), (1.0, 0.0, nan, 0.0),
                       (c, s, 1.0, nan), (nan, nan, 0.0, 0.0), (nan, 0.0, 1.0, 1.0), (inf, 0.0, 0.0, 0.0), (c, s, 1e300, 0.0), (1.0, 0.0, -1e300, 1e300),
                       (0.0, -1.0, 2.0, -1e300), pose(-1.0, -2.0, 1.0)])
    rng = np.random.Generator(np.random.PCG64(12))
    pos = np.column_stack([rng.uniform(-5.0, 5.0, 70), rng.uniform(-5.0, 5.0, 70), rng.uniform(0.0, 1.0, 70)])
    cat = _u32([1] * 66 + [2] * 3 + [3])
    det = np.array([(2.0, 0.5, 0.25), (1.0, -1.0, 0.5), (0.5, 2.0, 0.0), (3.0, 0.0, 0.75), (-1.0, 1.0, 0.25)])
    out = []
    for dcat in ([1, 2, 3, 1, 2], [1], [9, 9]):
        k = len(dcat)
        out.append(Case("not_finite_poses[landmark,k=%d]" % k, False, pos, cat, states, _w0(len(states), k), det[:k], _u32(dcat),
                        dict(sigma_range=1.5, sigma_bearing=1.25, random_prob=1e-3)))
        out.append(Case("not_finite_poses[bearing,k=%d]" % k, True, pos, cat, states, _w0(len(states), 10 + k), det[:k], _u32(dcat),
                        dict(sigma_bearing=1.25, sensor_pose_in_robot=TILTED)))
    return out


FAMILIES = {"near_ties": near_ties, "range_leaks": range_leaks, "degenerate_vectors": degenerate_vectors, "tiny_weights": tiny_weights,
            "far_maps": far_maps}
RULE_FAMILIES = {"overflow_underflow": overflow_underflow, "not_finite_poses": not_finite_poses}

# Where each mutant of landmark_reference.MUTANTS must die (test_landmark_reference_cpu.py asserts the table).
MUTANT_DIES_IN = {
    "fma_d2": "near_ties", "assoc_xy_z": "near_ties", "robot_frame": "near_ties", "last_of_equals": "near_ties", "wave_tie_to_larger": "near_ties",
    "drop_last_stride": "near_ties", "wave_no_pick_wins": "range_leaks", "range_first_minus_1": "range_leaks", "range_count_plus_1": "range_leaks",
    "count0_as_1": "range_leaks", "bearing_slot_collides": "range_leaks", "bearing_run_shared": "range_leaks",
}
# ... and the cases, by tag, on which it must: for the mutants of the arithmetic (the first three) pairs that the mutated sequence orders
# the other way, found by running it; for the others the cases whose construction names the fault - an `equal` pair, in two lanes of
# a group for the wave reduction; the later place 129 past the last whole stride of 64 lanes; a category of one landmark under 64
# lanes, 63 of which scan nothing; a bait before and behind a range; a category the map does not have; several bearing detections,
# and several of one category.
MUTANT_DIES_ON = {
    "fma_d2": ("near_ties[identity,origin,inverted,k=1,at=(5, 129),order=1]", "near_ties[identity,utm,inverted,k=8,at=(0, 8),order=0]"),
    "assoc_xy_z": ("near_ties[axis,utm,inverted,k=8,at=(64, 65),order=0]",),
    "robot_frame": ("near_ties[general,origin,ulp,k=2,at=(5, 129),order=0]", "near_ties[axis,utm,inverted,k=8,at=(64, 65),order=0]"),
    "last_of_equals": ("near_ties[identity,origin,equal,k=1,at=(0, 1),order=0]", "near_ties[general,utm,equal,k=33,at=(0, 1),order=1]"),
    "wave_tie_to_larger": ("near_ties[axis,origin,equal,k=1,at=(63, 64),order=0]", "near_ties[axis,utm,equal,k=8,at=(5, 129),order=1]"),
    "drop_last_stride": ("near_ties[identity,origin,inverted,k=1,at=(5, 129),order=1]",),
    "wave_no_pick_wins": ("range_leaks[landmark,k=1,start=0]", "range_leaks[bearing,k=1]"),
    "range_first_minus_1": ("range_leaks[landmark,k=1,start=1]", "range_leaks[bearing,k=64]"),
    "range_count_plus_1": ("range_leaks[landmark,k=1,start=1]", "range_leaks[bearing,k=64]"),
    "count0_as_1": ("range_leaks[landmark,k=1,start=2]", "range_leaks[bearing,k=5,absent]"),
    "bearing_slot_collides": ("range_leaks[bearing,k=3]",),
    "bearing_run_shared": ("range_leaks[bearing,k=64,one_category]",),
}
WAVE_ONLY = ("wave_tie_to_larger", "wave_no_pick_wins", "drop_last_stride")


def rule_bound(case, exponents):
    """The relative distance a device may keep from the loop form on a RULE family, per state: both run the same f64 operations in the
    same order, so they differ through sqrt, atan2 and exp alone, each within an ulp of the real function on either side (2 between
    them).  An aperture goes through two sqrt and one atan2 (6 ulps), a range error through one sqrt (2); squared, 12 ulps of the
    exponent at the most, which exp turns into 12 |exponent| ulps of the term, and its own 2.  Over a state: (12 sum |exponent| + 2 k)
    ulps for the terms, k + 1 for the product's roundings being the same ones on both sides but not the same operands."""
    return (12.0 * exponents + 3.0 * case.k + 1.0) * 2.0**-53
