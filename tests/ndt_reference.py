"""numpy f64 restatement of the reference's 2D NDT sensor model (beluga/include/beluga/sensor/ndt_sensor_model.hpp,
sensor/data/ndt_cell.hpp), the yardstick of tests/test_ndt_cpu.py and tests/test_gpu_ndt.py.

  to_cells(points, resolution)      detail::to_cells (:88-110) + fit_points (:66-80): groups by (p / resolution) truncated toward
                                    zero, groups of < 5 points dropped, mean + sample covariance with the diagonal clamped to 1e-5
  likelihood_at(map, params, m, c)  NDTSensorModel::likelihood_at (:229-239) of a measurement cell already in the map frame
  weights(map, params, states, cells)  operator() (:216-226): 1 + sum over the cells of likelihood_at(state * cell)
"""
import math

import numpy as np

DEFAULT_KERNEL = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 0), (0, 1), (1, -1), (1, 0), (1, 1))


def fit_points(pts):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    mean = pts.mean(axis=0)
    d = pts - mean
    cov = d.T @ d / (len(pts) - 1)
    cov[0, 0] = max(cov[0, 0], 1e-5)
    cov[1, 1] = max(cov[1, 1], 1e-5)
    return mean, cov


def to_cells(points, resolution):
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    groups = {}
    for p in pts:
        key = (int(p[0] / resolution), int(p[1] / resolution))  # Eigen cast<int>: truncation toward zero
        groups.setdefault(key, []).append(p)
    means, covs = [], []
    for key in sorted(groups):
        g = groups[key]
        if len(g) < 5:
            continue
        m, c = fit_points(g)
        means.append(m)
        covs.append(c)
    return np.asarray(means).reshape(-1, 2), np.asarray(covs).reshape(-1, 2, 2)


class NdtMap:
    def __init__(self, cells, means, covariances, resolution):
        self.resolution = float(resolution)
        self.data = {(int(k[0]), int(k[1])): (np.asarray(m, dtype=np.float64), np.asarray(c, dtype=np.float64).reshape(2, 2))
                     for k, m, c in zip(np.asarray(cells).reshape(-1, 2), np.asarray(means).reshape(-1, 2),
                                        np.asarray(covariances).reshape(-1, 2, 2))}

    def cell_near(self, p):  # regular_grid.hpp:75-78
        inv = 1.0 / self.resolution
        return int(math.floor(p[0] * inv)), int(math.floor(p[1] * inv))


def cell_likelihood(map_mean, map_cov, mean, cov, d1=1.0, d2=1.0):  # ndt_cell.hpp:49-54
    e = np.asarray(mean) - map_mean
    return d1 * math.exp((-d2 / 2.0) * float(e @ np.linalg.inv(np.asarray(cov) + map_cov) @ e))


def likelihood_at(ndt_map, mean, cov, minimum_likelihood=0.0, d1=1.0, d2=1.0, kernel=DEFAULT_KERNEL):
    cx, cy = ndt_map.cell_near(mean)
    total = 0.0
    for dx, dy in kernel:
        hit = ndt_map.data.get((cx + dx, cy + dy))
        if hit is not None:
            total += cell_likelihood(hit[0], hit[1], mean, cov, d1, d2)
    return max(total, minimum_likelihood)


def transform_cell(state, mean, cov):  # operator*(SE2, NDTCell), ndt_cell.hpp:61-66; state = (cos, sin, x, y)
    c, s, x, y = state
    R = np.array([[c, -s], [s, c]])
    return np.array([c * mean[0] - s * mean[1] + x, s * mean[0] + c * mean[1] + y]), R @ np.asarray(cov) @ R.T


def weights(ndt_map, states, means, covs, minimum_likelihood=0.0, d1=1.0, d2=1.0, kernel=DEFAULT_KERNEL):
    states = np.asarray(states, dtype=np.float64).reshape(-1, 4)
    out = np.empty(len(states))
    for i, st in enumerate(states):
        acc = 1.0
        for m, c in zip(means, covs):
            tm, tc = transform_cell(st, m, c)
            acc += likelihood_at(ndt_map, tm, tc, minimum_likelihood, d1, d2, kernel)
        out[i] = acc
    return out


def weights_vectorized(ndt_map, states, means, covs, minimum_likelihood=0.0, d1=1.0, d2=1.0, kernel=DEFAULT_KERNEL):
    """weights() over many states at once (numpy over the states; the same arithmetic, the cells and offsets in the same order)."""
    st = np.asarray(states, dtype=np.float64).reshape(-1, 4)
    c, s, x, y = st[:, 0], st[:, 1], st[:, 2], st[:, 3]
    keys = sorted(ndt_map.data)
    codes = np.array([(kx << 32) + (ky & 0xFFFFFFFF) for kx, ky in keys], dtype=np.int64)
    order = np.argsort(codes)
    codes = codes[order]
    mm = np.array([ndt_map.data[keys[i]][0] for i in order]).reshape(-1, 2)
    mc = np.array([ndt_map.data[keys[i]][1] for i in order]).reshape(-1, 2, 2)
    inv = 1.0 / ndt_map.resolution
    acc = np.ones(len(st))
    for m, cv in zip(means, covs):
        ux = c * m[0] - s * m[1] + x
        uy = s * m[0] + c * m[1] + y
        R = np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)  # (n, 2, 2)
        tc = R @ np.asarray(cv) @ np.transpose(R, (0, 2, 1))
        cx = np.floor(ux * inv).astype(np.int64)
        cy = np.floor(uy * inv).astype(np.int64)
        total = np.zeros(len(st))
        for dx, dy in kernel:
            code = ((cx + dx) << 32) + ((cy + dy) & 0xFFFFFFFF)
            pos = np.clip(np.searchsorted(codes, code), 0, len(codes) - 1) if len(codes) else np.zeros(len(st), dtype=np.int64)
            hit = (codes[pos] == code) if len(codes) else np.zeros(len(st), dtype=bool)
            if not np.any(hit):
                continue
            e = np.stack([ux - mm[pos, 0], uy - mm[pos, 1]], -1)[hit]
            S = tc[hit] + mc[pos[hit]]
            q = np.einsum("ni,nij,nj->n", e, np.linalg.inv(S), e)
            total[hit] += d1 * np.exp((-d2 / 2.0) * q)
        acc += np.maximum(total, minimum_likelihood)
    return acc
