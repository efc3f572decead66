"""numpy f64 restatement of the reference's landmark and bearing sensor models for 2D states
(beluga/include/beluga/sensor/landmark_sensor_model.hpp, bearing_sensor_model.hpp, sensor/data/landmark_map.hpp) and of the box
generator their contexts draw random states from, the yardstick of tests/test_landmark_cpu.py and tests/test_gpu_landmark.py.

  LandmarkMap(positions, categories, boundaries=None)   both constructors + map_limits()
  landmark_weights(map, states, detections, categories, sigma_range, sigma_bearing, random_prob)   -> (weights, gaps)
  bearing_weights(map, states, bearings, categories, sigma_bearing, sensor_pose_in_robot)          -> (weights, gaps)
  box_states(map, seed, step, indices)                  MultivariateUniformDistribution<SE2d, AlignedBox2d> over map_limits()

States are (cos, sin, x, y) and stand for Rz(theta), (x, y, 0); the rotation is applied from (cos, sin) directly.  3-vector sums
associate as v0 + (v1 + v2); the product over the detections as libstdc++'s transform_reduce: blocks of four, then one by one.
gaps[i, j] is how far particle i's match for detection j is from the runner-up: (d2_second - d2_best) / d2_second for the landmark
model, (dot_best - dot_second) / |detection| for the bearing model; candidates at the position of the match itself do not count
(whichever of them is picked, the term is the same), and inf where there is no runner-up.
"""
import dataclasses
import math
from fractions import Fraction

import mpmath
import numpy as np

from oracle import binding as orc

RNG_RANDOM_STATE, RNG_RANDOM_BOX_Y = 3, 8
IDENTITY_SE3 = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)  # Sophus::SE3d::data(): quaternion x, y, z, w, translation x, y, z


class LandmarkMap:
    def __init__(self, positions, categories, boundaries=None):
        self.positions = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
        self.categories = np.asarray(categories, dtype=np.uint32).reshape(-1)
        assert len(self.positions) == len(self.categories)
        if boundaries is None:  # landmark_map.hpp:61-71 (an empty map keeps Eigen's empty box; the library refuses that case)
            assert len(self.positions) > 0
            boundaries = (self.positions.min(axis=0), self.positions.max(axis=0))
        self.boundaries = (np.asarray(boundaries[0], dtype=np.float64), np.asarray(boundaries[1], dtype=np.float64))

    def map_limits(self):
        return self.boundaries

    def of_category(self, category):
        return self.positions[self.categories == np.uint32(category)]  # map order kept


def _norm3(x, y, z):
    return np.sqrt(x * x + (y * y + z * z))


def _normalized(x, y, z):
    """Eigen's normalized(): v / sqrt(squaredNorm), v itself where that is zero."""
    n2 = x * x + (y * y + z * z)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.sqrt(n2)
        pos = n2 > 0
        return np.where(pos, x / n, x), np.where(pos, y / n, y), np.where(pos, z / n, z)


def _aperture(ax, ay, az, bx, by, bz):
    """atan2(|a x b|, a . b)"""
    cos = ax * bx + (ay * by + az * bz)
    cx, cy, cz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
    return np.arctan2(_norm3(cx, cy, cz), cos)


def transform_reduce_product(terms):
    """std::transform_reduce(first, last, 1.0, multiplies, f) as libstdc++ evaluates it; terms: (k, n)."""
    acc = np.ones(terms.shape[1]) if len(terms) else 1.0
    j = 0
    while j + 4 <= len(terms):
        acc = acc * ((terms[j] * terms[j + 1]) * (terms[j + 2] * terms[j + 3]))
        j += 4
    while j < len(terms):
        acc = acc * terms[j]
        j += 1
    return acc


def _second(best, second, value, same_as_best):
    """Runner-up bookkeeping for a candidate that did not win: it counts unless it sits where the winner sits."""
    return np.where(same_as_best, second, np.minimum(second, value))


def landmark_weights(lmap, states, detections, categories, sigma_range=1.0, sigma_bearing=1.0, random_prob=1e-4):
    st = np.asarray(states, dtype=np.float64).reshape(-1, 4)
    det = np.asarray(detections, dtype=np.float64).reshape(-1, 3)
    c, s, x, y = st[:, 0], st[:, 1], st[:, 2], st[:, 3]
    n = len(st)
    den_r, den_b = (2.0 * sigma_range) * sigma_range, (2.0 * sigma_bearing) * sigma_bearing
    terms, gaps = np.zeros((len(det), n)), np.full((n, len(det)), np.inf)
    for j, (d, cat) in enumerate(zip(det, categories)):
        cand = lmap.of_category(cat)
        if len(cand) == 0:
            terms[j] = random_prob
            continue
        dr = float(_norm3(d[0], d[1], d[2]))
        dhx, dhy, dhz = (float(v) for v in _normalized(d[0], d[1], d[2]))
        px, py, pz = (c * d[0] - s * d[1]) + x, (s * d[0] + c * d[1]) + y, np.full(n, d[2])
        best = np.zeros(n)
        pick = np.zeros(n, dtype=np.int64)
        for t, l in enumerate(cand):  # std::min_element with <: the first of equal minima
            ex, ey, ez = l[0] - px, l[1] - py, l[2] - pz
            d2 = ex * ex + (ey * ey + ez * ez)
            better = d2 < best if t else np.ones(n, dtype=bool)
            best = np.where(better, d2, best)
            pick = np.where(better, t, pick)
        second = np.full(n, np.inf)
        for t, l in enumerate(cand):
            ex, ey, ez = l[0] - px, l[1] - py, l[2] - pz
            d2 = ex * ex + (ey * ey + ez * ez)
            second = _second(best, second, d2, np.all(cand[pick] == l, axis=1))
        with np.errstate(invalid="ignore", divide="ignore"):
            gaps[:, j] = np.where(np.isinf(second), np.inf, (second - best) / second)
        l = cand[pick]
        vx, vy, vz = l[:, 0] - x, l[:, 1] - y, l[:, 2]
        rx, ry, rz = c * vx + s * vy, c * vy - s * vx, vz
        lr = _norm3(rx, ry, rz)
        lhx, lhy, lhz = _normalized(rx, ry, rz)
        be = _aperture(lhx, lhy, lhz, dhx, dhy, dhz)
        re = dr - lr
        terms[j] = np.exp(-re * re / den_r) * np.exp(-be * be / den_b) + random_prob
    return transform_reduce_product(terms) * np.ones(n), gaps


def rotation_matrix(q):
    """Eigen's Quaternion::toRotationMatrix for (x, y, z, w)."""
    x, y, z, w = (float(v) for v in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def bearing_weights(lmap, states, bearings, categories, sigma_bearing=1.0, sensor_pose_in_robot=IDENTITY_SE3):
    st = np.asarray(states, dtype=np.float64).reshape(-1, 4)
    det = np.asarray(bearings, dtype=np.float64).reshape(-1, 3)
    c, s, x, y = st[:, 0], st[:, 1], st[:, 2], st[:, 3]
    n = len(st)
    pose = [float(v) for v in sensor_pose_in_robot]
    Rs, ts = rotation_matrix(pose[:4]), pose[4:]
    # sensor_in_world = robot * sensor: rotation Rz Rs, translation Rz ts + t
    R0 = [c * Rs[0][k] - s * Rs[1][k] for k in range(3)]
    R1 = [s * Rs[0][k] + c * Rs[1][k] for k in range(3)]
    R2 = [Rs[2][k] for k in range(3)]
    tx, ty, tz = (c * ts[0] - s * ts[1]) + x, (s * ts[0] + c * ts[1]) + y, ts[2]
    den_b = (2.0 * sigma_bearing) * sigma_bearing
    terms, gaps = np.zeros((len(det), n)), np.full((n, len(det)), np.inf)

    def bearing_of(l):  # normalized(sensor_in_world^-1 * l) = normalized(Rw^T (l - tw))
        v0, v1, v2 = l[..., 0] - tx, l[..., 1] - ty, l[..., 2] - tz
        return _normalized(*[R0[k] * v0 + (R1[k] * v1 + R2[k] * v2) for k in range(3)])

    for j, (d, cat) in enumerate(zip(det, categories)):
        cand = lmap.of_category(cat)
        if len(cand) == 0:
            terms[j] = 0.0
            continue
        best = np.zeros(n)
        pick = np.zeros(n, dtype=np.int64)
        dots = []
        for t, l in enumerate(cand):  # min_element with >: the first of equal maxima; the detection as given
            bx, by, bz = bearing_of(l)
            dot = bx * d[0] + (by * d[1] + bz * d[2])
            dots.append(dot)
            better = dot > best if t else np.ones(n, dtype=bool)
            best = np.where(better, dot, best)
            pick = np.where(better, t, pick)
        second = np.full(n, np.inf)
        for t, l in enumerate(cand):
            second = _second(best, second, best - dots[t], np.all(cand[pick] == l, axis=1))
        dn = float(_norm3(d[0], d[1], d[2]))
        with np.errstate(invalid="ignore", divide="ignore"):
            gaps[:, j] = np.where(np.isinf(second), np.inf, second / dn)
        bx, by, bz = bearing_of(cand[pick])
        dhx, dhy, dhz = (float(v) for v in _normalized(d[0], d[1], d[2]))
        e = _aperture(dhx, dhy, dhz, bx, by, bz)
        terms[j] = np.exp(-e * e / den_b)
    return transform_reduce_product(terms) * np.ones(n), gaps


def _u53(words, a, b):
    return float(((int(words[a]) << 32) | int(words[b])) >> 11) * 2.0 ** -53


def box_states(lmap, seed, step, indices):
    """x = min.x + (max.x - min.x) u_x, y likewise, heading -pi + 2 pi u_theta: purpose 3 words 0,1 -> u_x, words 2,3 -> u_theta,
    purpose 8 words 0,1 -> u_y; addressed by the candidate's global index and the cycle's step."""
    lo, hi = lmap.map_limits()
    out = np.zeros((len(indices), 4))
    for k, j in enumerate(indices):
        a = orc.draw(seed, step, RNG_RANDOM_STATE, int(j))
        b = orc.draw(seed, step, RNG_RANDOM_BOX_Y, int(j))
        theta = -math.pi + 2.0 * math.pi * _u53(a, 2, 3)
        out[k] = (math.cos(theta), math.sin(theta), lo[0] + (hi[0] - lo[0]) * _u53(a, 0, 1), lo[1] + (hi[1] - lo[1]) * _u53(b, 0, 1))
    return out


# ---- the exact yardstick, the f64 loop form and its mutants (tests/landmark_families.py, test_gpu_landmark_edges.py) ----------------------
# weights_loop is the kernels' sequence in plain Python floats (IEEE f64, one rounding per operation, libm's exp, atan2 and sqrt), record
# by record as landmark_layout_map and landmark_records lay them out: the landmarks grouped by category (stable), a record's (first,
# count, place), the bearing records sorted by category.  `wave` walks a record's range as the wave-per-particle kernels do - g lanes,
# lane r scanning first + r, first + r + g, ..., then the xor butterfly of group_reduce with pick_beats - and must return the lane form's
# bits.  A Variant switches ONE thing wrong; the families of landmark_families.py exist to tell each of them from the real sequence.
# weights_exact takes the pick of the unmutated sequence and evaluates everything behind it in 60-digit arithmetic from the f64 inputs
# as given ((c, s) is not renormalised; den = 2 sigma sigma exactly).
NO_PICK = 0xFFFFFFFF
MP_DIGITS = 60


@dataclasses.dataclass(frozen=True)
class Variant:
    fma_d2: bool = False              # squared_distance contracted: fma(ex, ex, fma(ey, ey, ez ez))
    assoc_xy_z: bool = False          # squared_distance as (x + y) + z
    robot_frame: bool = False         # the distance measured in the robot frame: |R^T (l - t) - d|^2
    last_of_equals: bool = False      # <= in place of < (>= for the dot products)
    wave_tie_to_larger: bool = False  # group_reduce: an equal value goes to the LARGER index
    wave_no_pick_wins: bool = False   # group_reduce: a lane that scanned nothing wins the step
    drop_last_stride: bool = False    # the strided scan stops at the last whole stride
    range_first_minus_1: bool = False  # a record's range starts one landmark early
    range_count_plus_1: bool = False   # ... ends one landmark late
    count0_as_1: bool = False         # a category the map does not have resolves to the next one's first landmark (a lower_bound without ==)
    bearing_slot_collides: bool = False  # the bearing term's slot is place modulo k - 1
    bearing_run_shared: bool = False     # the detections of a run share the run head's search state


PLAIN = Variant()
MUTANTS = {f.name: Variant(**{f.name: True}) for f in dataclasses.fields(Variant)}


def fma(a, b, c):
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # (Fraction -> float rounds once, to nearest even)


def layout(lmap):
    """landmark_layout_map's grouping: the positions sorted by category (stable), the sorted categories, {category: (first, count)}."""
    order = np.argsort(lmap.categories, kind="stable")
    cats = lmap.categories[order]
    ranges = {}
    for i, c in enumerate(cats.tolist()):
        first, count = ranges.get(c, (i, 0))
        ranges[c] = (first, count + 1)
    return lmap.positions[order], cats, ranges


def records(lmap, categories, bearing, variant=PLAIN):
    """landmark_records' plumbing: [(first, count, place)] in record order - the caller's for the landmark model, sorted by category
    (stable) for the bearing model."""
    _, cats, ranges = layout(lmap)
    categories = np.asarray(categories, dtype=np.uint32)
    order = np.argsort(categories, kind="stable") if bearing else np.arange(len(categories))
    out = []
    for i in order.tolist():
        first, count = ranges.get(int(categories[i]), (NO_PICK, 0))
        if count == 0 and variant.count0_as_1 and len(cats):
            first, count = min(int(np.searchsorted(cats, categories[i], side="left")), len(cats) - 1), 1
        if count and variant.range_first_minus_1:
            first, count = first - 1, count + 1
        if count and variant.range_count_plus_1:
            count += 1
        out.append((first, count, i))
    return out


def _landmark_at(grouped, index):
    """(a mutant's read beside the buffer sees zeros)"""
    index &= 0xFFFFFFFF
    return tuple(float(v) for v in grouped[index]) if index < len(grouped) else (0.0, 0.0, 0.0)


def _sq3(x, y, z):
    return x * x + (y * y + z * z)


def _dot3(a, b):
    return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])


def _unit(v):
    n2 = _sq3(*v)
    if not n2 > 0.0:
        return v
    n = math.sqrt(n2)
    return (v[0] / n, v[1] / n, v[2] / n)


def _aperture_f64(a, b):
    cross = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
    return math.atan2(math.sqrt(_sq3(*cross)), _dot3(a, b))


def group_of(k):
    g = 64
    while 64 // g < k:
        g //= 2
    return g


def _better(v, best, larger, variant):
    if variant.last_of_equals:
        return v >= best if larger else v <= best
    return v > best if larger else v < best


def _beats(v, at, ov, oat, larger, variant):
    if variant.wave_no_pick_wins and oat == NO_PICK:
        return False
    if oat == NO_PICK:
        return True
    if at == NO_PICK:
        return False
    if v == ov:
        return at > oat if variant.wave_tie_to_larger else at < oat
    return v > ov if larger else v < ov


def pick_of(values, larger, variant=PLAIN, g=None):
    """The place in its category of the candidate the scan selects; g: the lanes of the wave kernel's group (None: the lane kernel)."""
    count = len(values)
    if g is None:
        best, at = values[0], 0
        for t in range(1, count):
            if _better(values[t], best, larger, variant):
                best, at = values[t], t
        return at
    limit = count - count % g if variant.drop_last_stride and count >= g else count
    lane_v, lane_at = [0.0] * g, [NO_PICK] * g
    for r in range(g):
        for t in range(r, limit, g):
            if t == r or _better(values[t], lane_v[r], larger, variant):
                lane_v[r], lane_at[r] = values[t], t
    step = g >> 1
    while step >= 1:
        nv, na = list(lane_v), list(lane_at)
        for lane in range(g):
            o = lane ^ step
            if not _beats(lane_v[lane], lane_at[lane], lane_v[o], lane_at[o], larger, variant):
                nv[lane], na[lane] = lane_v[o], lane_at[o]
        lane_v, lane_at, step = nv, na, step >> 1
    return lane_at[0]


def world_point(state, d):
    c, s, x, y = state
    return ((c * d[0] - s * d[1]) + x, (s * d[0] + c * d[1]) + y, d[2])


def squared_distance(l, p, variant=PLAIN, state=None, d=None):
    if variant.robot_frame:
        c, s, x, y = state
        vx, vy = l[0] - x, l[1] - y
        ex, ey, ez = (c * vx + s * vy) - d[0], (c * vy - s * vx) - d[1], l[2] - d[2]
    else:
        ex, ey, ez = l[0] - p[0], l[1] - p[1], l[2] - p[2]
    if variant.fma_d2:
        return fma(ex, ex, fma(ey, ey, ez * ez))
    if variant.assoc_xy_z:
        return (ex * ex + ey * ey) + ez * ez
    return ex * ex + (ey * ey + ez * ez)


def _product(terms):
    acc, j = 1.0, 0
    while j + 4 <= len(terms):
        acc = acc * ((terms[j] * terms[j + 1]) * (terms[j + 2] * terms[j + 3]))
        j += 4
    while j < len(terms):
        acc = acc * terms[j]
        j += 1
    return acc


def sensor_frame(state, Rs, ts):
    c, s, x, y = state
    R = [0.0] * 9
    for k in range(3):
        R[k], R[3 + k], R[6 + k] = c * Rs[0][k] - s * Rs[1][k], s * Rs[0][k] + c * Rs[1][k], Rs[2][k]
    return R, ((c * ts[0] - s * ts[1]) + x, (s * ts[0] + c * ts[1]) + y, ts[2])


def _bearing_of(frame, l):
    R, t = frame
    v = (l[0] - t[0], l[1] - t[1], l[2] - t[2])
    return _unit(tuple(R[k] * v[0] + (R[3 + k] * v[1] + R[6 + k] * v[2]) for k in range(3)))


def weights_loop(lmap, states, detections, categories, w0, bearing=False, sigma_range=1.0, sigma_bearing=1.0, random_prob=1e-4,
                 sensor_pose_in_robot=IDENTITY_SE3, variant=PLAIN, wave=False):
    """-> (weights[n], picks[n][k], exponents[n]): w0 times the product of the terms in the kernels' f64 sequence; picks[i][j] is the
    place of the match in its category for the detection at the caller's place j (None without a landmark); exponents[i] is the sum of
    the magnitudes of every exp argument of state i."""
    st = np.asarray(states, dtype=np.float64).reshape(-1, 4)
    det = [tuple(float(v) for v in d) for d in np.asarray(detections, dtype=np.float64).reshape(-1, 3)]
    k = len(det)
    grouped, _, _ = layout(lmap)
    recs = records(lmap, categories, bearing, variant)
    g = group_of(k) if wave and k else None
    den_r, den_b = (2.0 * sigma_range) * sigma_range, (2.0 * sigma_bearing) * sigma_bearing
    pose = [float(v) for v in sensor_pose_in_robot]
    Rs, ts = rotation_matrix(pose[:4]).tolist(), pose[4:]
    out, picks, exponents = np.zeros(len(st)), [], np.zeros(len(st))
    for i, row in enumerate(st):
        state = tuple(float(v) for v in row)
        c, s, x, y = state
        terms, pk, big = [1.0] * k, [None] * k, 0.0
        if not bearing:
            for first, count, place in recs:
                d = det[place]
                if count == 0:
                    terms[place] = random_prob
                    continue
                p = world_point(state, d)
                at = pick_of([squared_distance(_landmark_at(grouped, first + t), p, variant, state, d) for t in range(count)], False, variant, g)
                pk[place] = at
                l = _landmark_at(grouped, first + at)
                vx, vy = l[0] - x, l[1] - y
                in_robot = (c * vx + s * vy, c * vy - s * vx, l[2])
                be = _aperture_f64(_unit(in_robot), _unit(d))
                re = math.sqrt(_sq3(*d)) - math.sqrt(_sq3(*in_robot))
                a, b = -re * re / den_r, -be * be / den_b
                big += abs(a) + abs(b)
                terms[place] = math.exp(a) * math.exp(b) + random_prob
        else:
            frame = sensor_frame(state, Rs, ts)
            head = None
            for n_rec, (first, count, place) in enumerate(recs):
                d = det[place]
                slot = place % (k - 1) if variant.bearing_slot_collides and k > 1 else place
                if count == 0:
                    terms[slot], head = 0.0, None
                    continue
                at = pick_of([_dot3(_bearing_of(frame, _landmark_at(grouped, first + t)), d) for t in range(count)], True, variant, g)
                if variant.bearing_run_shared:
                    if head is not None and head[0] == first:
                        at = head[1]
                    head = (first, at)
                pk[place] = at
                e = _aperture_f64(_unit(d), _bearing_of(frame, _landmark_at(grouped, first + at)))
                a = -e * e / den_b
                big += abs(a)
                terms[slot] = math.exp(a)
        out[i] = float(w0[i]) * _product(terms)
        picks.append(pk)
        exponents[i] = big
    return out, picks, exponents


def _mp(v):
    return mpmath.mpf(float(v))


def _mp_unit(v):
    n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    if n2 == 0:
        return v
    n = mpmath.sqrt(n2)
    return [v[0] / n, v[1] / n, v[2] / n]


def _mp_aperture(a, b):
    cross = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    sin, cos = mpmath.sqrt(cross[0] * cross[0] + cross[1] * cross[1] + cross[2] * cross[2]), a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    return mpmath.mpf(0) if sin == 0 and cos == 0 else mpmath.atan2(sin, cos)


def weights_exact(lmap, states, detections, categories, w0, bearing=False, sigma_range=1.0, sigma_bearing=1.0, random_prob=1e-4,
                  sensor_pose_in_robot=IDENTITY_SE3):
    """-> (weights as mpf[n], picks): the match by the f64 sequence (weights_loop's, unmutated: the first of equal ones in map order, v0 +
    (v1 + v2), world frame, the bearing search with the detection as given); the robot-frame landmark, the norms, normalized(), the
    aperture, both exponentials, + random_prob, the product and the prior weight in MP_DIGITS-digit arithmetic from the f64 inputs as
    given.  normalized() of a vector whose squared norm is exactly zero is the vector, and atan2(0, 0) = 0, as in the kernel and Eigen."""
    st = np.asarray(states, dtype=np.float64).reshape(-1, 4)
    det = np.asarray(detections, dtype=np.float64).reshape(-1, 3)
    grouped, _, _ = layout(lmap)
    recs = records(lmap, categories, bearing)
    _, picks, _ = weights_loop(lmap, st, det, categories, w0, bearing, sigma_range, sigma_bearing, random_prob, sensor_pose_in_robot)
    with mpmath.workdps(MP_DIGITS):
        den_r, den_b = 2 * _mp(sigma_range) * _mp(sigma_range), 2 * _mp(sigma_bearing) * _mp(sigma_bearing)
        rp = _mp(random_prob)
        qx, qy, qz, qw = (_mp(v) for v in sensor_pose_in_robot[:4])
        Rs = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
              [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
              [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]]
        ts = [_mp(v) for v in sensor_pose_in_robot[4:]]
        units = [_mp_unit([_mp(v) for v in d]) for d in det]
        ranges = [mpmath.sqrt(sum(_mp(v) * _mp(v) for v in d)) for d in det]
        out = []
        for i, row in enumerate(st):
            c, s, x, y = (_mp(v) for v in row)
            acc, memo = _mp(w0[i]), {}
            if bearing:
                Rw = [[c * Rs[0][k] - s * Rs[1][k] for k in range(3)], [s * Rs[0][k] + c * Rs[1][k] for k in range(3)], Rs[2]]
                tw = [c * ts[0] - s * ts[1] + x, s * ts[0] + c * ts[1] + y, ts[2]]
            for first, count, place in recs:
                if count == 0:
                    acc = acc * (0 if bearing else rp)
                    continue
                key = (first + picks[i][place], tuple(det[place]))
                if key not in memo:
                    l = [_mp(v) for v in grouped[first + picks[i][place]]]
                    if bearing:
                        v = [l[0] - tw[0], l[1] - tw[1], l[2] - tw[2]]
                        b = _mp_unit([Rw[0][k] * v[0] + Rw[1][k] * v[1] + Rw[2][k] * v[2] for k in range(3)])
                        e = _mp_aperture(units[place], b)
                        memo[key] = mpmath.exp(-e * e / den_b)
                    else:
                        vx, vy = l[0] - x, l[1] - y
                        in_robot = [c * vx + s * vy, c * vy - s * vx, l[2]]
                        lr = mpmath.sqrt(in_robot[0] * in_robot[0] + in_robot[1] * in_robot[1] + in_robot[2] * in_robot[2])
                        be = _mp_aperture(_mp_unit(in_robot), units[place])
                        re = ranges[place] - lr
                        memo[key] = mpmath.exp(-re * re / den_r) * mpmath.exp(-be * be / den_b) + rp
                acc = acc * memo[key]
            out.append(acc)
    return out, picks


DENORMAL_STEP = mpmath.mpf(2) ** -1074


def excess_errors(got, exact, absolute_steps=0):
    """max(|got - exact| - absolute_steps 2^-1074, 0) / exact per weight, in MP_DIGITS digits; a weight that is not finite gives inf,
    and so does any difference from an exact 0."""
    out = np.zeros(len(got))
    with mpmath.workdps(MP_DIGITS):
        for i, (g, e) in enumerate(zip(got, exact)):
            if not math.isfinite(g):
                out[i] = math.inf
                continue
            over = abs(mpmath.mpf(float(g)) - e) - absolute_steps * DENORMAL_STEP
            out[i] = 0.0 if over <= 0 else (math.inf if e == 0 else float(over / e))
    return out
