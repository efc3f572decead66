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
import math

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
